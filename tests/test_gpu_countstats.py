"""GPU tests of include/dpmm_hip_countstats.h (csrc/countstats.hip) and of host/score.py's Predictor.count_statistics / absorb_counts.

The reference is numpy Float64 (tests/tools/countstats_ref.py) on what the library's own `predict` and `score_samples` return for the
same data and Predictor: the classes of the points, N and sums by W' X, and the magnitude T1 the bound is stated in.  Counters are
compared exactly; integer data with hard weights against the Int64 evaluation bit for bit, and across the byte, Float32, strided device
and sparse stores; everything else by |got - ref| <= 2 gamma(n + 2) (T1, N_ref), gamma(m) = m u / (1 - m u), u = 2^-53 -- it holds for
any order of the additions and fails if w x was rounded to Float32.  Models are made through Predictor._setup from posteriors written by
hand, no fit.  One sweep per axis around the base shape D = 8, K = 5, n = 1000: D over the 64-feature blocks, the 256-feature
workgroups and the 128-byte rows of the byte store (dense), and over one and several 7168-feature ranges of the sparse kernel up to
D = 65536; K over the 16-cluster tile and the 64-cluster group of the score kernels; n across the 64-point batch, the 256-point walk and
several chunks of 2048; capacities 64, 1000 and beyond n; one table budget that cuts an upload into several ranges."""
import importlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import test_gpu_score as S
from tools import countstats_ref as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ("hard", "soft")


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


def same_stats(a, b):
    return all(same(x, y) for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:]


def posterior(D, K, rng):
    """Dirichlet posteriors written by hand: every cluster prefers its own features."""
    alpha = 0.25 + rng.integers(0, 8, (K, D)) / 4.0                                      # dyadic: exact in Float32
    for k in range(K):
        alpha[k, k % D] += 16.0
    return dict(alpha=alpha.astype(np.float32))


def open_predictor(host, post, cap, counts=None, no_u8=False, binding=None):
    K, D = post["alpha"].shape
    p = host.Predictor.__new__(host.Predictor)
    p._setup(1, D, 10.0, np.full(K, 100.0) if counts is None else counts, post, cap, 0, None)
    if no_u8:
        p._wk.set_option(binding.OPT_MULT_NO_U8, 1)                                      # before any points: the Float32 store for integer counts
    return p


def counts_data(post, n, rng, trials=12):
    """(D, n) float32 of small integer counts drawn from the clusters."""
    a = post["alpha"].astype(np.float64)
    z = rng.integers(0, a.shape[0], n)
    pr = a[z] / a[z].sum(1, keepdims=True)
    return np.stack([rng.multinomial(trials, q) for q in pr]).T.astype(np.float32)


def sparse_data(D, n, rng, integer=True):
    """scipy CSC (D, n): 0 .. 6 entries per point (some points have none), point 0 holds rows 0 and D - 1."""
    cnt = rng.integers(0, min(7, D + 1), n)
    cnt[0] = min(2, D)
    if n > 3:
        cnt[3] = 0
    rows = [np.sort(rng.choice(D, c, replace=False)) for c in cnt]
    rows[0] = np.array([0, D - 1][:cnt[0]])
    val = [rng.integers(1, 6, c).astype(np.float32) * (1.0 if integer else np.float32(0.1)) for c in cnt]
    cp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return sp.csc_matrix((np.concatenate(val).astype(np.float32), np.concatenate(rows).astype(np.int64), cp), shape=(D, n))


def torch_csc(X):
    return torch.sparse_csc_tensor(torch.from_numpy(X.indptr.astype(np.int64)), torch.from_numpy(X.indices.astype(np.int64)), torch.from_numpy(X.data),
                                   size=X.shape).to(DEV)


def reference(p, X, floor=None, model_X=None):
    """{mode: the definitions on `predict`'s and `score_samples`' output for the same data, same Predictor}, logdens, (labels, P)."""
    lab, P = (as_np(a) for a in p.predict(X))
    ld = as_np(p.score_samples(X))
    Xm = X if model_X is None else model_X
    return {mode: C.stats(Xm, lab, P, mode, ld, floor) for mode in MODES}, ld, (lab, P)


def check(got, want, n, mode, what="", exact=None):
    """got: a CountStatistics; want: the reference of the same mode; exact: (N, sums) Int64 when the data are integers (hard mode)."""
    K, D = got.sums.shape
    assert got.N.dtype == got.sums.dtype == np.float64 and got.count.dtype == np.int64 and got.N.shape == got.count.shape == (K,)
    w = C.within(got, want, n)
    print(what, mode, "K", K, "D", D, "n", n, "largest difference in units of the bound 2 gamma(n + 2) T1:", w)
    assert np.array_equal(got.count, want["count"]), what
    assert (got.skipped, got.incomplete, got.held_out) == (want["skipped"], want["incomplete"], want["held_out"]), what
    assert int(got.count.sum()) + got.skipped + got.incomplete + got.held_out == n, what
    assert w <= 1, (what, w)
    if mode == "hard":
        assert np.array_equal(got.N, got.count.astype(np.float64)), what
        if exact is not None:
            assert same(got.N, exact[0].astype(np.float64)) and same(got.sums, exact[1].astype(np.float64)), what
    else:
        assert abs(got.N.sum() - got.count.sum()) <= n * K * 2.0 ** -23, what                        # rows of probabilities sum to 1


def run_case(host, post, X, cap, what, integer=True, model_X=None, mb=None, binding=None, no_u8=False):
    """Both modes of one input through one Predictor against its own predict; model_X: the same points for the reference."""
    Xm = X if model_X is None else model_X
    n = Xm.shape[1]
    with open_predictor(host, post, cap, no_u8=no_u8, binding=binding) as p:
        want, ld, (lab, P) = reference(p, X, model_X=Xm)
        ex = C.exact(Xm, lab, P) if integer else None
        if mb is not None:
            p._wk.set_option(binding.OPT_SCORE_TABLE_MB, mb)
        out = {}
        for mode in MODES:
            out[mode] = p.count_statistics(X, assign=mode)
            check(out[mode], want[mode], n, mode, what, ex)
    return out, want


# ------------------------------------------------------------------------------------------------ the stores
def test_every_store_and_identical_sums_for_integer_counts(host, binding):
    D, K, n = 8, 5, 1000
    rng = np.random.default_rng(1)
    post = posterior(D, K, rng)
    X = counts_data(post, n, rng)
    Xs = sp.csc_matrix(X)
    wide = torch.zeros((D, 2 * n), dtype=torch.float32, device=DEV)
    wide[:, ::2] = torch.from_numpy(X).to(DEV)
    outs = {}
    outs["byte"], _ = run_case(host, post, X, 256, "byte store")
    outs["float32"], _ = run_case(host, post, X, 256, "Float32 store of integers", no_u8=True, binding=binding)
    outs["strided"], _ = run_case(host, post, wide[:, ::2], 256, "strided device tensor", model_X=X)
    outs["sparse"], _ = run_case(host, post, Xs, 256, "scipy CSC")
    outs["tuple"], _ = run_case(host, post, (Xs.indptr.astype(np.int64), Xs.indices.astype(np.int64), Xs.data, Xs.shape), 256, "CSC tuple", model_X=Xs)
    outs["torch"], _ = run_case(host, post, torch_csc(Xs), 256, "torch.sparse_csc on the device", model_X=Xs)
    assert (outs["byte"]["hard"].count > 0).sum() >= 2
    for name, o in outs.items():
        assert all(isinstance(v, np.ndarray) for v in o["hard"][:3]), name
        assert same_stats(o["hard"], outs["byte"]["hard"]), name                                     # exact: one value whatever the store


@pytest.mark.parametrize("extra", [0.5, 0.1])       # halves are bf16-exact but no bytes; tenths are neither
def test_float32_store_of_values_that_are_no_integers(host, extra):
    D, K, n = 8, 5, 1000
    rng = np.random.default_rng(2)
    post = posterior(D, K, rng)
    X = counts_data(post, n, rng) + np.float32(extra) * (rng.random((D, n)) < 0.3)
    run_case(host, post, X.astype(np.float32), 256, ("extra", extra), integer=False)


# ------------------------------------------------------------------------------------------------ one sweep per axis
@pytest.mark.parametrize("D", [1, 3, 64, 65, 127, 128, 129, 300])
def test_every_block_layout_of_dense_D(host, D):
    rng = np.random.default_rng(10 + D)
    post = posterior(D, 5, rng)
    X = counts_data(post, 1000, rng)
    out, _ = run_case(host, post, X, 1000, ("byte D", D))
    assert out["hard"].sums[:, D - 1].sum() == X[D - 1].sum()                                        # the last feature arrives
    run_case(host, post, X + np.float32(0.1) * (rng.random(X.shape) < 0.2).astype(np.float32), 1000, ("float32 D", D), integer=False)


@pytest.mark.parametrize("D", [300, 5000, 65536])
def test_sparse_D_up_to_the_widest(host, D):
    rng = np.random.default_rng(20 + D % 1000)
    post = posterior(D, 5, rng)
    X = sparse_data(D, 1000, rng)
    out, _ = run_case(host, post, X, 1000, ("sparse D", D))
    dense_col = np.asarray(X.sum(1)).ravel()
    assert np.array_equal(out["hard"].sums.sum(0), dense_col) and out["hard"].sums[:, D - 1].sum() > 0 and out["hard"].sums[:, 0].sum() > 0
    assert (np.diff(X.indptr) == 0).sum() > 0 and out["hard"].count.sum() == 1000                    # the points without entries are counted
    if D == 300:
        run_case(host, post, sparse_data(D, 1000, rng, integer=False), 1000, ("sparse tenths D", D), integer=False)


@pytest.mark.parametrize("K", [1, 2, 5, 16, 17, 65])
def test_every_K(host, K):
    rng = np.random.default_rng(30 + K)
    post = posterior(8, K, rng)
    run_case(host, post, counts_data(post, 1000, rng), 1000, ("byte K", K))
    post = posterior(300, K, rng)
    run_case(host, post, sparse_data(300, 1000, rng), 1000, ("sparse K", K))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 5000])
def test_n_across_batches_and_chunks(host, n):
    rng = np.random.default_rng(40 + n)
    post = posterior(8, 5, rng)
    run_case(host, post, counts_data(post, n, rng), n, ("byte n", n))
    X = counts_data(post, n, rng) + np.float32(0.1)
    run_case(host, post, X, n, ("float32 n", n), integer=False)
    post = posterior(300, 5, rng)
    run_case(host, post, sparse_data(300, n, rng), n, ("sparse n", n))


def test_capacities_and_ranges_of_a_small_table_budget_agree(host, binding):
    D, K, n = 8, 5, 1000
    rng = np.random.default_rng(50)
    post = posterior(D, K, rng)
    for name, X in (("byte", counts_data(post, n, rng)), ("sparse", sparse_data(D, n, rng))):
        outs = {cap: run_case(host, post, X, cap, (name, "capacity", cap))[0] for cap in (64, 1000, 1500)}
        assert S.tile_of("mult", D) < n                                                              # budget 0: ranges of one tile, several per upload
        outs["ranges"], want = run_case(host, post, X, 1000, (name, "one-tile ranges"), mb=0.0, binding=binding)
        for key in (64, 1500, "ranges"):
            assert same_stats(outs[key]["hard"], outs[1000]["hard"]), (name, key)                    # exact: to the bit
            a, b = outs[1000]["soft"], outs[key]["soft"]
            assert np.array_equal(a.count, b.count) and a[3:] == b[3:], (name, key)
            assert C.within(b, dict(want["soft"], N=a.N, sums=a.sums), n) <= 1, (name, key)          # within the bound of each other


def test_the_same_call_gives_the_same_bits_and_a_second_pass_allocates_nothing(host):
    rng = np.random.default_rng(60)
    post = posterior(17, 5, rng)
    Xd = torch.from_numpy((counts_data(post, 5000, rng) + np.float32(0.1)).T.copy()).to(DEV).T     # (D, n) view of point-major memory: read in place
    Xs = torch_csc(sparse_data(17, 5000, rng, integer=False))
    with open_predictor(host, post, 2048) as p:
        for name, X in (("dense", Xd), ("sparse", Xs)):
            for mode in MODES:
                a = p.count_statistics(X, assign=mode)
                torch.cuda.synchronize()
                before = torch.cuda.mem_get_info(0)[0]
                b = p.count_statistics(X, assign=mode)
                torch.cuda.synchronize()
                assert torch.cuda.mem_get_info(0)[0] == before, (name, mode)
                assert same_stats(a, b) and a.count.sum() == 5000, (name, mode)


# ------------------------------------------------------------------------------------------------ points that take no part
def test_values_that_are_not_finite_add_nothing(host):
    D, K, n = 8, 5, 1000
    rng = np.random.default_rng(70)
    post = posterior(D, K, rng)
    X = counts_data(post, n, rng)
    bad = [7, 130, 258, 300]
    X[0, 7] = np.nan
    X[2, 130] = np.nan
    X[1, 258] = np.inf
    X[:, 300] = np.nan
    with open_predictor(host, post, 256) as p:
        want, _, _ = reference(p, X)
        clean = None
        for mode in MODES:
            got = p.count_statistics(X, assign=mode)
            check(got, want[mode], n, mode, "dense with NaN")
            assert got.skipped + got.incomplete == len(bad)
        clean = p.count_statistics(np.delete(X, bad, axis=1))                                        # the same points without the four
        assert np.array_equal(clean.count, want["hard"]["count"]) and (clean.skipped, clean.incomplete) == (0, 0)
        assert C.within(clean, want["hard"], n) <= 1
    Xs = sparse_data(300, n, rng).tolil()
    Xs[5, 11] = np.nan
    Xs[299, 400] = np.inf
    Xs = Xs.tocsc()
    post = posterior(300, K, rng)
    with open_predictor(host, post, 256) as p:
        want, _, _ = reference(p, Xs)
        for mode in MODES:
            got = p.count_statistics(Xs, assign=mode)
            check(got, want[mode], n, mode, "sparse with NaN")
            assert got.skipped + got.incomplete == 2 and np.isfinite(got.sums).all()


def test_min_logdens_at_the_median_holds_half_out(host):
    D, K, n = 8, 5, 1000
    rng = np.random.default_rng(80)
    post = posterior(D, K, rng)
    for name, X in (("byte", counts_data(post, n, rng)), ("sparse", sp.csc_matrix(counts_data(post, n, rng)))):
        with open_predictor(host, post, 256) as p:
            ld = as_np(p.score_samples(X))
            thr = float(np.median(ld))
            want, _, (lab, P) = reference(p, X, floor=thr)
            for mode in MODES:
                got = p.count_statistics(X, assign=mode, min_logdens=thr)
                check(got, want[mode], n, mode, (name, "floor"), C.exact(X, lab, P, ld, thr))
                assert got.held_out == int((ld < np.float32(thr)).sum()) and 300 < got.held_out < 700 and got.skipped == 0
            assert p.count_statistics(X, min_logdens=-np.inf).held_out == 0 and p.count_statistics(X, min_logdens=np.inf).held_out == n


def test_the_zero_padding_of_a_short_slab_takes_no_part(host):
    D, K, n, cap = 8, 4, 261, 256
    rng = np.random.default_rng(90)
    post = posterior(D, K, rng)
    X = counts_data(post, n, rng)
    with open_predictor(host, post, cap) as p:
        want, _, (lab, P) = reference(p, X)
        for mode in MODES:
            check(p.count_statistics(X, assign=mode), want[mode], n, mode, "short slab", C.exact(X, lab, P))
        wk = p._wk
        wk.countstats_begin(0)
        wk.countstats_accumulate(cap)                                                                # what the worker holds now, whole: 5 points and 251 rows of zeros
        padded = wk.countstats_read()
        assert padded["count"].sum() == cap and padded["sums"].sum() == X[:, 256:].sum()


# ------------------------------------------------------------------------------------------------ absorb
def separated(D, K):
    """Clusters on disjoint features: a batch of a few hundred points moves no label, yet it outweighs the posterior it is folded into."""
    alpha = np.full((K, D), 0.5, np.float32)
    for k in range(K):
        alpha[k, 2 * k:2 * k + 2] = 64.0
    return dict(alpha=alpha)


def test_absorb_counts_updates_the_served_model(host, pkg, tmp_path):
    D, K, n = 12, 4, 600
    rng = np.random.default_rng(110)
    post = separated(D, K)
    counts = rng.integers(50, 500, K).astype(np.float64)
    X = counts_data(post, n, rng)
    Y = counts_data(post, 300, rng)
    for mode in MODES:
        with open_predictor(host, post, 256, counts=counts) as p:
            before = p.score_samples(Y)
            drawn = p.sample(40, seed=3, trials=20)                                                  # the sampler's tables of the old posterior are loaded
            wk = p._wk
            wk.overlap_begin()                                                                       # an accumulation under the old parameters
            want = p.count_statistics(X, assign=mode)
            got = p.absorb_counts(X, assign=mode)
            assert same_stats(got, want)
            with pytest.raises(pkg.DpmmError) as e:
                wk.overlap_accumulate(wk.n)
            assert e.value.code == -4 and "changed" in str(e.value)                                  # DPMM_ESTATE: the predictives were reloaded
            assert p.post["alpha"].dtype == np.float64
            hit = got.N > 0
            ref = post["alpha"].astype(np.float64)
            ref[hit] += got.sums[hit]
            assert same(p.post["alpha"], ref) and same(p.points_count, counts + np.where(hit, got.N, 0.0))
            assert p._sampler_set is False                                                           # the alias tables are stale
            after = p.predict(Y)
            assert not same(before, p.score_samples(Y))                                              # the model moved
            with open_predictor(host, p.post, 256, counts=p.points_count) as fresh:                  # ... to exactly the absorbed posterior:
                wanted = fresh.predict(Y)                                                            # the worker was really reloaded
                fresh_draw = fresh.sample(40, seed=3, trials=20)
            assert same(after[0], wanted[0]) and same(after[1], wanted[1])
            redrawn = p.sample(40, seed=3, trials=20)                                                # `sample` uses the new posterior
            assert same(redrawn[0], fresh_draw[0]) and same(redrawn[1], fresh_draw[1]) and not same(redrawn[0], drawn[0])
            if mode == "hard":                                                                       # the same integer batch once more: alpha0 + 2 sums
                again = p.absorb_counts(X, assign=mode)
                assert same_stats(again, got)
                assert same(p.post["alpha"], post["alpha"].astype(np.float64) + 2 * got.sums)
                after = p.predict(Y)
            path = str(tmp_path / f"{mode}.npz")
            p.save(path)
            snap = p.post["alpha"].copy()
            none = p.absorb_counts(np.full((D, 30), np.nan, np.float32), assign=mode)                # nobody takes part: no bit changes
            assert none.count.sum() == 0 and none.N.sum() == 0 and same(p.post["alpha"], snap)
            for call in (p.statistics, p.absorb):                                                    # the NIW calls still refuse
                with pytest.raises(ValueError, match="NIW"):
                    call(X)
        with host.Predictor.load(path, capacity=64) as q:
            loaded = q.predict(Y)
            assert same(q.post["alpha"], snap) and q.post["alpha"].dtype == np.float64
        assert same(loaded[0], after[0]) and same(loaded[1], after[1])


# ------------------------------------------------------------------------------------------------ calls
def test_refusals_come_before_any_launch(pkg):
    n, D = 300, 8
    rng = np.random.default_rng(3)
    wk = pkg.Worker(pkg.PRIOR_MULT, D, n, device=0, seed=1)
    wk.upload_points(rng.poisson(0.8, (n, D)).astype(np.float32))

    def refused(code, fn, *a, what=(), **kw):
        with pytest.raises(pkg.DpmmError) as e:
            fn(*a, **kw)
        assert e.value.code == code, str(e.value)
        for w in what:
            assert w in str(e.value), str(e.value)

    def params(K):
        logp, w = S.mult_params(rng, D, K)
        return logp, w

    refused(-4, wk.countstats_begin)                                    # DPMM_ESTATE: no predictive parameters yet
    refused(-4, wk.countstats_accumulate, n)                            # no dpmm_countstats_begin
    refused(-4, wk.countstats_read_raw)
    with pytest.raises((RuntimeError, pkg.DpmmError)):
        wk.countstats_read()
    wk.set_predictive_mult(*params(3))
    refused(-4, wk.countstats_accumulate, n)                            # a refused begin starts nothing
    refused(-1, wk.countstats_begin, 2, what=("mode",))
    wk.countstats_begin(1, -1e9)
    refused(-1, wk.countstats_accumulate, n + 1, what=("n_valid",))
    refused(-1, wk.countstats_accumulate, -1, what=("n_valid",))
    assert wk._lib.dpmm_countstats_read(wk._h, None) == -1              # out == NULL
    wk.countstats_accumulate(n)
    wk.countstats_accumulate(0)                                         # nothing
    got = wk.countstats_read()
    assert got["count"].sum() + got["held_out"][0] == n and got["skipped"][0] == 0 and got["incomplete"][0] == 0
    wk.set_predictive_mult(*params(4))                                 # another K than begin saw
    refused(-4, wk.countstats_accumulate, n, what=("changed",))
    wk.countstats_begin(0)
    wk.set_predictive_mult(*params(4))                                 # the same K, other parameters
    refused(-4, wk.countstats_accumulate, n, what=("changed",))
    r = wk.countstats_read()
    assert r["count"].sum() == 0 and not r["sums"].any() and not r["N"].any()      # nothing was launched: the accumulators are as begin left them
    wk.close()
    niw = pkg.Worker(pkg.PRIOR_NIW, 2, n, device=0, seed=1)
    refused(-1, niw.countstats_begin, what=("Multinomial",))            # DPMM_EINVAL, whatever its state
    niw.close()
