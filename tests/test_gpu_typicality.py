"""GPU tests of include/dpmm_hip_typicality.h (csrc/typicality.hip) and of host/score.py's Predictor.typicality / min_tail.

The reference is numpy Float64 (tests/tools/typicality_ref.py) from the Float32 m, R, df the worker is given.  Models are made through
Predictor._setup from posteriors written by hand (tests/tools/sample_ref.py's niw_model), no fit: D in {2, 17, 64, 256}, K in {1, 3, 40},
n = 1000 and a few placed points, df cycling over {4, 300, 1e7} across the clusters; capacities 384 (a short last slab) and 1000, and a
table budget of 0 MB (ranges of one tile).

  q      |q - ref| <= 4 (D + 2) 2^-24 a_i, a_i = sum_r (sum_c |R_rc| |z_c|)^2: each y_r carries at most gamma(D + 1) sum_c |R_rc| |z_c|
         (the rounding of z included), the sum of squares adds gamma(D); together under (3 D + 4) u a_i.
  tail   against betainc(df / 2, D / 2, df / (df + q)) in Float64 on the RETURNED q: relative 2^-20 wherever the reference is at least
         1e-30 (one Float32 rounding, 6e-8, plus the reference's own log-beta cancellation, 7e7 2^-52 at df = 1e7); at most 2e-30 below.

One departure from the issue's list of cases: it asks for a row with a +Inf feature to be counted in `incomplete` under "propagate".  By the
issue's own definitions (and by tests/test_gpu_batchstats.py) such a row has no finite entry -- R has a positive diagonal, so q is Inf
under every cluster -- and is SKIPPED; `incomplete` is reached through missing="marginalize" only.  The test asserts the definitions."""
import importlib

import numpy as np
import pytest
import torch

import test_gpu_score as S
from tools import sample_ref as SR
from tools import typicality_ref as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DFS = (4.0, 300.0, 1e7)
SIGMAS = (1.0, 10.0, 11.7, 100.0)


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def binding(pkg):
    return importlib.import_module(pkg.__name__ + ".binding")


@pytest.fixture(scope="module")
def host(pkg):
    return importlib.import_module(pkg.__name__ + ".host")


def as_np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def same(a, b):
    """Equal shapes, types and bits."""
    a, b = np.ascontiguousarray(as_np(a)), np.ascontiguousarray(as_np(b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_typ(a, b):
    return all(same(x, y) for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:]


def model(D, K, seed):
    """(post, m, A, df): df cycles over DFS; the cluster centres are spread so that most points keep the cluster they were drawn from."""
    df = np.array([DFS[k % 3] for k in range(K)])
    post, m, A, df = SR.niw_model(D, K, df, seed)
    post["m"] = m = (m * 4.0).astype(np.float32).astype(np.float64)
    return post, m, A, df


def open_predictor(host, post, cap, **kw):
    K, D = post["m"].shape
    p = host.Predictor.__new__(host.Predictor)
    p._setup(0, D, 10.0, np.full(K, 100.0), post, cap, 0, None, **kw)
    return p


def points(m, A, n, rng):
    """(D, n + extras) Float32: n draws around the centres, then every centre itself, then the centres moved by SIGMAS predictive
    standard deviations along the last column of A (y = s e_D: q = s^2); returns (X, index of the first centre, of the first moved point)."""
    K, D = m.shape
    z = rng.integers(0, K, n)
    x = m[z] + np.einsum("nij,nj->ni", A[z], rng.standard_normal((n, D)))
    far = np.concatenate([m + s * A[:, :, D - 1] for s in SIGMAS])
    return np.concatenate([x, m, far]).T.astype(np.float32), n, n + K


def worker_params(p):
    which, (m, R, logdet, df, w) = p._predictive_args()
    return T.worker_params(m, R, df)


def check(got, X, params, what):
    """Properties 1-3 of one result against the reference; returns the reference tails."""
    lab, q, tail = (as_np(a) for a in got[:3])
    D, n = X.shape
    assert lab.dtype == np.int64 and q.dtype == np.float32 and tail.dtype == np.float32 and lab.shape == q.shape == tail.shape == (n,)
    ok = ~np.isnan(q)
    assert int((~ok).sum()) == got.skipped + got.incomplete and np.array_equal(np.isnan(tail), ~ok), what
    qr, a, _ = T.reference(X[:, ok], lab[ok] - 1, *params)
    err = np.abs(q[ok].astype(np.float64) - qr)
    bound = 4 * (D + 2) * 2.0 ** -24 * a
    print(what, "D", D, "largest |q - ref| in units of the bound:", float((err / np.maximum(bound, 1e-300)).max()))
    assert np.all(q[ok] >= 0) and np.all(np.isfinite(q[ok])) and np.all(err <= bound), what
    tr = T.tail_of(q[ok].astype(np.float64), params[2].astype(np.float64)[lab[ok] - 1], D)
    t = tail[ok].astype(np.float64)
    big = tr >= 1e-30
    rel = np.abs(t[big] - tr[big]) / tr[big]
    print(what, "largest relative tail error:", float(rel.max()), "in units of 2^-20:", float(rel.max() * 2 ** 20), "tails below 1e-30:", int((~big).sum()))
    assert np.all(rel <= 2.0 ** -20) and np.all(t[~big] <= 2e-30) and np.all((t >= 0) & (t <= 1)), what
    assert np.all(t[q[ok] == 0] == 1.0), what
    return tr


# ------------------------------------------------------------------------------------------------ every shape
@pytest.mark.parametrize("K", [1, 3, 40])
@pytest.mark.parametrize("D", [2, 17, 64, 256])
def test_labels_q_and_tail_at_every_shape(host, binding, D, K):
    rng = np.random.default_rng(1000 * D + K)
    post, m, A, df = model(D, K, 7 * D + K)
    X, c0, f0 = points(m, A, 1000, rng)
    n = X.shape[1]
    out = {}
    for cap in (384, 1000):
        with open_predictor(host, post, cap) as p:
            params = worker_params(p)
            out[cap] = p.typicality(X)
            assert same(out[cap].labels, p.predict_labels(X)), cap                                   # 1: the labels of predict_labels, to the bit
            if cap == 1000:
                assert S.tile_of("niw", D) < cap
                p._wk.set_option(binding.OPT_SCORE_TABLE_MB, 0.0)                                    # ranges of one tile, several per upload
                out["ranges"] = p.typicality(X)
    got = out[384]
    assert (got.skipped, got.incomplete) == (0, 0)
    tr = check(got, X, params, ("K", K))
    assert same_typ(out[384], out[1000]) and same_typ(out[1000], out["ranges"])                      # 4: capacities and budgets, to the bit
    lab, q, tail = (as_np(a) for a in got[:3])
    # the centres: every one that keeps its own label sits at q = 0, tail = 1 exactly
    own = lab[c0:f0] == np.arange(1, K + 1)
    assert own.sum() >= 1 and np.all(q[c0:f0][own] == 0) and np.all(tail[c0:f0][own] == 1)
    # both branches of the continued fraction
    a_, b_ = 0.5 * params[2].astype(np.float64)[lab - 1], 0.5 * D
    x_ = 2 * a_ / (2 * a_ + q.astype(np.float64))
    direct = x_ < (a_ + 1) / (a_ + b_ + 2)
    assert direct.any() and (~direct).any()


@pytest.mark.parametrize("D", [2, 17])
@pytest.mark.parametrize("df", [300.0, 1e7])
def test_tails_on_either_side_of_1e_30(host, D, df):
    """One light-tailed cluster, so that far points keep its label: the centre moved by 1, 10, 11.7, 12, 13 and 100 predictive standard
    deviations along every column of A (q = s^2 up to the rounding of x; at D = 2, df = 1e7 the tail is exp(-q / 2): 1.9e-30 at 11.7,
    5.4e-32 at 12)."""
    post, m, A, dfs = SR.niw_model(D, 1, df, 40 + D)
    X = np.concatenate([m + s * A[0].T for s in (0.0, 1.0, 10.0, 11.7, 12.0, 13.0, 100.0)]).T.astype(np.float32)      # rows of A' = columns of A
    with open_predictor(host, post, 64) as p:
        got = p.typicality(X)
        tr = check(got, X, worker_params(p), ("far", D, df))
    q, tail = as_np(got.mahalanobis), as_np(got.tail)
    assert np.allclose(q.reshape(7, D)[1:], np.array([1.0, 100.0, 11.7 ** 2, 144.0, 169.0, 1e4])[:, None], rtol=1e-3)
    assert np.all(tail[:D] == 1) and np.all(np.diff(tail.reshape(7, D), axis=0) <= 0)                # exactly 1 at the centre, non-increasing in s
    if D == 2 and df == 1e7:
        assert ((tr < 1e-30) & (tr > 1e-40)).any() and ((tr >= 1e-30) & (tr < 1e-28)).any()


# ------------------------------------------------------------------------------------------------ every kind of input
def test_host_array_device_tensor_and_a_bfloat16_view_agree(host):
    D, K, n = 17, 3, 1000
    rng = np.random.default_rng(5)
    post, m, A, df = model(D, K, 50)
    X, _, _ = points(m, A, n, rng)
    bf = torch.from_numpy(X.T.copy()).to(DEV).to(torch.bfloat16)                                     # contiguous (n, D); .T is the (D, n) view
    xh = np.ascontiguousarray(bf.float().cpu().numpy().T)                                            # the same values as a host array
    with open_predictor(host, post, 384) as p:
        a = p.typicality(xh)
        assert all(isinstance(v, np.ndarray) for v in a[:3]) and isinstance(a.skipped, int) and isinstance(a.incomplete, int)
        check(a, xh, worker_params(p), "host array")
        for name, x in (("float32 tensor", torch.from_numpy(xh).to(DEV)), ("bfloat16 .T view", bf.T)):
            b = p.typicality(x)
            assert all(torch.is_tensor(v) and v.device == torch.device(DEV) for v in b[:3]), name
            assert same_typ(a, b), name


def test_projected_data_equals_its_transform(host):
    D, K, n, D_in = 8, 3, 600, 40
    rng = np.random.default_rng(6)
    post, m, A, df = model(D, K, 60)
    X, _, _ = points(m, A, n, rng)
    proj = host.random_projection(D_in, D, seed=3)
    Xs = (proj.basis @ X.astype(np.float64)).astype(np.float32)                                      # (D_in, n) source rows
    Z = as_np(proj.transform(Xs))                                                                    # the coordinates the worker computes
    with open_predictor(host, post, 256, projection=proj) as p:
        a, b = p.typicality(Xs), p.typicality(Z)
        assert same_typ(a, b)
        check(a, Z, worker_params(p), "projected")


# ------------------------------------------------------------------------------------------------ the classes
def test_skipped_and_incomplete_points(host):
    D, K, n = 6, 3, 1000
    rng = np.random.default_rng(7)
    post, m, A, df = model(D, K, 70)
    X, _, _ = points(m, A, n, rng)
    n = X.shape[1]
    clean = X.copy()
    X[0, 7] = np.nan                                                                                 # one gap
    X[2, 500] = np.nan
    X[1, 100] = np.inf                                                                               # no finite entry in its row
    X[:, 300] = np.nan                                                                               # nothing left to marginalise over
    gaps, lost = [7, 500], [100, 300]
    rest = np.setdiff1d(np.arange(n), gaps + lost)
    with open_predictor(host, post, 384) as p:
        base = p.typicality(clean)
        got = p.typicality(X)
        assert (got.skipped, got.incomplete) == (len(gaps) + len(lost), 0)                           # propagate: NaN and Inf poison the row
        q, t = as_np(got.mahalanobis), as_np(got.tail)
        assert np.isnan(q[gaps + lost]).all() and np.isnan(t[gaps + lost]).all() and same(got.labels, p.predict_labels(X))
        assert all(same(as_np(x)[rest], as_np(y)[rest]) for x, y in zip(got[:3], base[:3]))          # every other point untouched
    with open_predictor(host, post, 384, missing="marginalize") as p:
        got = p.typicality(X)
        assert (got.skipped, got.incomplete) == (len(lost), len(gaps)) and p.missing_counts[0] == len(gaps)
        q, t, lab = as_np(got.mahalanobis), as_np(got.tail), as_np(got.labels)
        assert np.isnan(q[gaps + lost]).all() and np.isnan(t[gaps + lost]).all()
        assert same(got.labels, p.predict_labels(X)) and np.all(lab[gaps] >= 1)                      # the gap points are labelled
        assert all(same(as_np(x)[rest], as_np(y)[rest]) for x, y in zip(got[:3], base[:3]))


# ------------------------------------------------------------------------------------------------ calibration, end to end
@pytest.mark.parametrize("D,df,seed", [(2, 4.0, 1), (64, 1e5, 2)])
def test_tails_of_the_models_own_draws_are_uniform(host, D, df, seed):
    """`sample` is counter-based: the seed decides the outcome once and for all.  KS distance under the 1 % critical distance."""
    n = 20000
    post, m, A, dfs = SR.niw_model(D, 1, df, 900 + D)
    with open_predictor(host, post, 8192) as p:
        x, _ = p.sample(n, seed=seed)
        got = p.typicality(x)
    d = T.ks_uniform(as_np(got.tail))
    print(f"D = {D} df = {df:g} seed = {seed}: KS distance {d:.5f}, critical {1.63 / np.sqrt(n):.5f}")
    assert (got.skipped, got.incomplete) == (0, 0) and d < 1.63 / np.sqrt(n)


# ------------------------------------------------------------------------------------------------ statistics / absorb with min_tail
def same_stats(a, b):
    return all(same(x, y) for x, y in zip(a[:4], b[:4])) and a[4:] == b[4:]


def test_min_tail_holds_out_exactly_the_points_below_it(host, tmp_path):
    D, K, n = 5, 3, 1000
    rng = np.random.default_rng(8)
    post, m, A, df = model(D, K, 80)
    X, _, _ = points(m, A, n, rng)
    X[1, 11] = np.nan                                                                                # a skipped point
    n = X.shape[1]
    t = 0.25
    with open_predictor(host, post, 384) as p:                                                       # a short last slab: the counters, exactly
        tail = as_np(p.typicality(X).tail)
        cut = p.statistics(X, min_tail=t)
        assert (cut.held_out, cut.skipped, cut.incomplete) == (int((tail < np.float32(t)).sum()), 1, 0)
    with open_predictor(host, post, 1100) as p:                                                      # one slab, one chunk: removing points keeps the order of the rest
        typ = p.typicality(X)
        assert same(typ.tail, tail)
        tail = as_np(typ.tail)
        out = tail < np.float32(t)                                                                   # (NaN compares false: the skipped point is not held out)
        plain = p.statistics(X)
        assert same_stats(plain, p.statistics(X, min_tail=None))                                     # None: the bits of a call without the keyword
        for mode in ("hard", "soft"):
            got = p.statistics(X, assign=mode, min_tail=t)
            assert got.held_out == int(out.sum()) > 50 and got.skipped == 1 and got.incomplete == 0, mode
            assert int(got.count.sum()) + got.held_out + got.skipped == n
            if mode == "hard":
                assert same_stats(got._replace(held_out=0), p.statistics(X[:, ~out]))                # the data with those points removed, to the bit
        ld = as_np(p.score_samples(X))
        floor = float(np.nanmedian(ld))
        both = p.statistics(X, min_logdens=floor, min_tail=t)
        scored = ~np.isnan(tail)                                                                     # (the skipped point's log-density is -Inf)
        assert both.held_out == int((out | ((ld < np.float32(floor)) & scored)).sum()) > got.held_out      # the union
        assert p.statistics(X, min_tail=1.0).held_out == int((tail < 1).sum())
        # absorb with the floor, then save / load: the updated model is served
        Y = X[:, :200]
        before = p.predict(Y)
        absorbed = p.absorb(X, min_tail=t)
        assert absorbed.held_out == int(out.sum())
        after = p.predict(Y)
        assert not same(before[1], after[1])
        path = str(tmp_path / "served.npz")
        p.save(path)
    with host.Predictor.load(path, capacity=1100) as q:
        loaded = q.predict(Y)
        assert same(loaded[0], after[0]) and same(loaded[1], after[1])
        assert q.typicality(Y).skipped == 1


def test_min_tail_under_marginalize_leaves_gap_points_incomplete(host):
    D, K, n = 6, 3, 500
    rng = np.random.default_rng(9)
    post, m, A, df = model(D, K, 90)
    X, _, _ = points(m, A, n, rng)
    X[0, 7] = np.nan
    with open_predictor(host, post, 256, missing="marginalize") as p:
        tail = as_np(p.typicality(X).tail)
        got = p.statistics(X, min_tail=1.0)                                                          # every complete point but those at a centre is held out
        assert got.incomplete == 1 and got.skipped == 0 and got.held_out == int((tail < 1).sum())


# ------------------------------------------------------------------------------------------------ calls
def test_refusals_come_before_any_launch(pkg):
    n = 300
    rng = np.random.default_rng(3)
    wk = pkg.Worker(pkg.PRIOR_NIW, 2, n, device=0, seed=1)
    wk.upload_points(rng.standard_normal((n, 2)).astype(np.float32))
    lab, q = np.zeros(n, np.int64), np.zeros(n, np.float32)

    def refused(code, fn, *a, what=(), **kw):
        with pytest.raises(pkg.DpmmError) as e:
            fn(*a, **kw)
        assert e.value.code == code, str(e.value)
        for w in what:
            assert w in str(e.value), str(e.value)

    refused(-4, wk.typicality_points_raw, False, labels=lab.ctypes.data)          # DPMM_ESTATE: no predictive parameters yet
    refused(-4, wk.batchstats_set_min_tail, 0.5)                                   # no dpmm_batchstats_begin
    wk.set_predictive_niw(*S.niw_params(rng, 2, 3))
    refused(-1, wk.typicality_points_raw, False)                                   # DPMM_EINVAL: every pointer null
    refused(-1, wk.typicality_points_raw, True, mahalanobis=q.ctypes.data, what=("mahalanobis",))      # host memory given as device memory
    assert wk._lib.dpmm_typicality_points(wk._h, None) == -1
    assert wk.typicality_points_into(dict(labels=lab, mahalanobis=q)) == (0, 0) and lab.min() >= 1 and np.all(q >= 0)
    wk.batchstats_begin(0)
    refused(-1, wk.batchstats_set_min_tail, 0.0, what=("min_tail",))
    refused(-1, wk.batchstats_set_min_tail, float("nan"), what=("min_tail",))
    wk.batchstats_set_min_tail(0.5)
    wk.batchstats_set_min_tail(None)
    wk.batchstats_accumulate(n)
    refused(-4, wk.batchstats_set_min_tail, 0.5, what=("first",))                  # DPMM_ESTATE: after the first accumulate
    assert wk.batchstats_read()["held_out"][0] == 0
    wk.close()
    mult = pkg.Worker(pkg.PRIOR_MULT, 8, n, device=0, seed=1)
    refused(-1, mult.typicality_points_raw, False, labels=lab.ctypes.data, what=("Multinomial",))      # DPMM_EINVAL, whatever its state
    mult.close()
