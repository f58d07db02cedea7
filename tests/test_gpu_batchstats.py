"""GPU tests of include/dpmm_hip_batchstats.h (csrc/batchstats.hip) and of host/score.py's Predictor.statistics / absorb.

The reference is numpy Float64 (tests/tools/batchstats_ref.py) on what the library's own `predict` and `score_samples` return for the
same data: the classes of the points, N, sums and S by einsum, and the magnitudes T, T1 the bound is stated in.  Every comparison of
the sums is |got - ref| <= 2 gamma(n + 2) (N_ref, T1, T), gamma(m) = m u / (1 - m u), u = 2^-53 -- it holds for any order of the
additions, fused or not, and fails if w x was rounded to Float32; the counters are compared exactly, the symmetry bit for bit.  Models
are made through Predictor._setup from posteriors written by hand, no fit.  One sweep per axis around the base shape D = 3, K = 5,
n = 1000: D over the padding of the rows (2, 3), one block of 64 features (17, 64), two (65) and every pair of four (256); K over 1, 2,
5 and 65 (more than one group of the score kernels' 64); n across the 64-point batch, the 256-point walk and several chunks of 2048
(1, 63, 64, 65, 1000, 5000); capacities 64, 1000 and beyond n."""
import importlib

import numpy as np
import pytest
import torch

import test_gpu_score as S
from tools import batchstats_ref as B

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
    return all(same(x, y) for x, y in zip(a[:4], b[:4])) and a[4:] == b[4:]


def posterior(D, K, rng):
    U = np.triu(rng.standard_normal((K, D, D)) * 0.1) + 2 * np.eye(D)
    nu = D + 3 + 50 * rng.random(K)
    return dict(kappa=1 + 50 * rng.random(K), nu=nu, m=rng.standard_normal((K, D)) * 3, U=U, logdet_psi=2 * np.log(np.einsum("kii->ki", U)).sum(1) - D * np.log(nu))


def open_predictor(host, post, cap, counts=None, **kw):
    """A Predictor of posteriors written by hand."""
    K, D = post["m"].shape
    p = host.Predictor.__new__(host.Predictor)
    p._setup(0, D, 10.0, np.full(K, 100.0) if counts is None else counts, post, cap, 0, None, **kw)
    return p


def blobs(post, n, rng, spread=1.5):
    K, D = post["m"].shape
    return (post["m"][rng.integers(0, K, n)] + spread * rng.standard_normal((n, D))).T.astype(np.float32)      # (D, n)


def reference(p, X, floor=None, model_X=None):
    """{mode: the definitions on `predict`'s and `score_samples`' output for the same data, same Predictor}; model_X: the points as the
    model sees them, when `X` is projected on the way in."""
    lab, P = p.predict(X)
    ld = p.score_samples(X)
    Xm = as_np(X if model_X is None else model_X).astype(np.float32)
    return {mode: B.stats(Xm, as_np(lab), as_np(P), mode, as_np(ld), floor) for mode in MODES}, as_np(ld)


def check(got, want, n, mode, what=""):
    """got: a BatchStatistics; want: the reference of the same mode; n: the points accumulated."""
    K, D = got.sums.shape
    assert got.N.dtype == got.sums.dtype == got.S.dtype == np.float64 and got.count.dtype == np.int64 and got.S.shape == (K, D, D)
    w = B.within(got, want, n)
    print(what, mode, "K", K, "D", D, "n", n, "largest difference in units of the bound 2 gamma(n + 2) T:", w)
    assert np.array_equal(got.count, want["count"]), what
    assert (got.skipped, got.incomplete, got.held_out) == (want["skipped"], want["incomplete"], want["held_out"]), what
    assert int(got.count.sum()) + got.skipped + got.incomplete + got.held_out == n, what
    assert w <= 1, (what, w)
    assert same(got.S, got.S.transpose(0, 2, 1).copy()), what                                        # symmetric bit for bit
    if mode == "hard":
        assert np.array_equal(got.N, got.count.astype(np.float64)), what
    else:
        assert abs(got.N.sum() - got.count.sum()) <= n * K * 2.0 ** -23, what                        # rows of probabilities sum to 1


def run_case(host, D, K, n, cap, seed, what, mb=None, binding=None):
    rng = np.random.default_rng(seed)
    post = posterior(D, K, rng)
    X = blobs(post, n, rng)
    with open_predictor(host, post, cap) as p:
        want, _ = reference(p, X)
        if mb is not None:
            p._wk.set_option(binding.OPT_SCORE_TABLE_MB, mb)
        out = {}
        for mode in MODES:
            out[mode] = p.statistics(X, assign=mode)
            check(out[mode], want[mode], n, mode, what)
    return out, want


# ------------------------------------------------------------------------------------------------ one sweep per axis
@pytest.mark.parametrize("D", [2, 3, 17, 64, 65, 256])
def test_every_block_layout_of_D(host, D):
    out, _ = run_case(host, D, 5, 1000, 1000, 10 + D, ("D", D))
    assert (out["hard"].count > 0).sum() >= 2
    if D == 256:
        assert np.abs(out["hard"].S[:, 192:, :64]).min() > 0 and np.abs(out["soft"].S[:, 255, :]).min() > 0      # the last block pair, the last row


@pytest.mark.parametrize("K", [1, 2, 5, 65])
def test_every_K(host, K):
    run_case(host, 3, K, 1000, 1000, 20 + K, ("K", K))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 5000])
def test_n_across_batches_and_chunks(host, n):
    run_case(host, 3, 5, n, n, 30 + n, ("n", n))


def test_capacities_agree_and_ranges_of_a_small_table_budget(host, binding):
    D, K, n = 3, 5, 1000
    outs = {cap: run_case(host, D, K, n, cap, 40, ("capacity", cap))[0] for cap in (64, 1000, 1500)}
    assert S.tile_of("niw", D) < n                                                                   # budget 0: ranges of one tile, four per upload
    outs["ranges"], want = run_case(host, D, K, n, 1000, 40, "one-tile ranges", mb=0.0, binding=binding)
    for mode in MODES:
        a = outs[1000][mode]
        for key in (64, 1500, "ranges"):
            b = outs[key][mode]
            assert np.array_equal(a.count, b.count) and a[4:] == b[4:], (mode, key)
            assert B.within(b, dict(want[mode], N=a.N, sums=a.sums, S=a.S), n) <= 1, (mode, key)      # within the bound of each other


def test_the_same_call_gives_the_same_bits_and_a_second_pass_allocates_nothing(host):
    rng = np.random.default_rng(50)
    post = posterior(17, 5, rng)
    X = torch.from_numpy(blobs(post, 5000, rng).T.copy()).to(DEV).T                                 # (D, n) view of point-major memory: read in place
    with open_predictor(host, post, 2048) as p:
        for mode in MODES:
            a = p.statistics(X, assign=mode)
            torch.cuda.synchronize()
            before = torch.cuda.mem_get_info(0)[0]
            b = p.statistics(X, assign=mode)
            torch.cuda.synchronize()
            assert torch.cuda.mem_get_info(0)[0] == before, mode
            assert same_stats(a, b), mode


# ------------------------------------------------------------------------------------------------ points that take no part
def gappy(post, n, rng):
    X = blobs(post, n, rng)
    D = X.shape[0]
    X[0, 7] = np.nan
    X[2, 130] = np.nan
    X[1, 258] = np.nan
    X[3, 258] = np.nan
    X[1, 100] = np.inf
    X[2, 64] = -np.inf
    X[:, 300] = np.nan                                                                               # nothing left to marginalise over
    assert D >= 4
    return X, [7, 130, 258], [100, 64, 300]


def test_nan_and_inf_features_propagate_and_marginalize(host):
    D, K, n = 6, 5, 1000
    rng = np.random.default_rng(60)
    post = posterior(D, K, rng)
    X, gaps, lost = gappy(post, n, rng)
    with open_predictor(host, post, 256) as p:                                                       # propagate: a NaN or Inf feature poisons the row
        want, _ = reference(p, X)
        for mode in MODES:
            got = p.statistics(X, assign=mode)
            check(got, want[mode], n, mode, "propagate")
            assert got.skipped == len(gaps) + len(lost) and got.incomplete == 0
    with open_predictor(host, post, 256, missing="marginalize") as p:                                # the gaps are labelled, their moments unknown
        want, _ = reference(p, X)
        for mode in MODES:
            got = p.statistics(X, assign=mode)
            check(got, want[mode], n, mode, "marginalize")
            assert got.incomplete == len(gaps) and got.skipped == len(lost)
        assert p.missing_counts[0] == len(gaps)
        clean = p.statistics(np.delete(X, gaps + lost, axis=1))                                      # the same points without the six
        assert np.array_equal(clean.count, got.count) and (clean.skipped, clean.incomplete) == (0, 0)
        assert B.within(clean, want["hard"], n) <= 1


def test_the_zero_padding_of_a_short_slab_takes_no_part(host):
    D, K, n, cap = 4, 4, 261, 256
    rng = np.random.default_rng(70)
    post = posterior(D, K, rng)
    post["m"][0] = 0.0                                                                               # the padding sits at the mean of cluster 1
    X = blobs(post, n, rng, spread=1.0)
    with open_predictor(host, post, cap) as p:
        want, _ = reference(p, X)
        for mode in MODES:
            check(p.statistics(X, assign=mode), want[mode], n, mode, "short slab")
        wk = p._wk
        wk.batchstats_begin(0)
        wk.batchstats_accumulate(cap)                                                                # what the worker holds now, whole: 5 points and 251 rows of zeros
        padded = wk.batchstats_read()
        assert padded["count"].sum() == cap and padded["count"][0] >= cap - 5


def test_min_logdens_at_the_median_holds_half_out(host):
    D, K, n = 3, 5, 1000
    rng = np.random.default_rng(80)
    post = posterior(D, K, rng)
    X = blobs(post, n, rng, spread=2.5)
    with open_predictor(host, post, 256) as p:
        ld = as_np(p.score_samples(X))
        thr = float(np.median(ld))
        want, _ = reference(p, X, floor=thr)
        for mode in MODES:
            got = p.statistics(X, assign=mode, min_logdens=thr)
            check(got, want[mode], n, mode, "floor")
            assert got.held_out == int((ld < np.float32(thr)).sum()) and 400 < got.held_out < 600 and got.skipped == 0
        assert p.statistics(X, min_logdens=-np.inf).held_out == 0 and p.statistics(X, min_logdens=np.inf).held_out == n


# ------------------------------------------------------------------------------------------------ every kind of input
def test_all_five_input_kinds(host):
    D, K, n = 8, 6, 2 * 256 + 5
    rng = np.random.default_rng(90)
    post = posterior(D, K, rng)
    bf = torch.from_numpy(blobs(post, n, rng).T.copy()).to(DEV).to(torch.bfloat16)                   # contiguous (n, D); .T is the (D, n) view
    xh = np.ascontiguousarray(bf.float().cpu().numpy().T)                                            # the same values as a host array
    wide = torch.zeros((D, 2 * n), dtype=torch.float32, device=DEV)
    wide[:, ::2] = torch.from_numpy(xh).to(DEV)
    with open_predictor(host, post, 256) as p:
        want, _ = reference(p, xh)
        for mode in MODES:
            a = p.statistics(xh, assign=mode)
            check(a, want[mode], n, mode, "host array")
            for name, x in (("float32 tensor", torch.from_numpy(xh).to(DEV)), ("bfloat16 .T view", bf.T), ("strided tensor", wide[:, ::2])):
                b = p.statistics(x, assign=mode)
                assert all(isinstance(v, np.ndarray) for v in b[:4]) and same_stats(a, b), (name, mode)
    D_in = 40
    proj = host.random_projection(D_in, D, seed=3)
    Xs = (proj.basis @ xh.astype(np.float64)).astype(np.float32)                                     # (D_in, n) source rows
    Z = as_np(proj.transform(Xs))                                                                    # the coordinates the worker computes
    with open_predictor(host, post, 256, projection=proj) as p:
        want, _ = reference(p, Xs, model_X=Z)
        for mode in MODES:
            got = p.statistics(Xs, assign=mode)
            check(got, want[mode], n, mode, "projected")
            assert same_stats(got, p.statistics(Z, assign=mode))                                     # d-row data is taken as already projected
        assert (got.count > 0).sum() >= 2


# ------------------------------------------------------------------------------------------------ absorb
def test_absorb_updates_the_served_model(host, pkg, tmp_path):
    D, K, n = 5, 4, 1000
    rng = np.random.default_rng(110)
    post = posterior(D, K, rng)
    counts = rng.integers(50, 500, K).astype(np.float64)
    X = blobs(post, n, rng)
    Y = blobs(post, 300, rng)
    for mode in MODES:
        with open_predictor(host, post, 256, counts=counts) as p:
            lab, P = (as_np(a) for a in p.predict(X))
            before = p.predict(Y)
            wk = p._wk
            wk.overlap_begin()                                                                       # an accumulation under the old parameters
            got = p.absorb(X, assign=mode)
            with pytest.raises(pkg.DpmmError) as e:
                wk.overlap_accumulate(wk.n)
            assert e.value.code == -4 and "changed" in str(e.value)                                  # DPMM_ESTATE: the predictives were reloaded
            # the reference update, centred, from the weights `predict` gave; tolerance as tests/test_batchstats_cpu.py measures it
            W = np.eye(K)[lab - 1] if mode == "hard" else P.astype(np.float64)
            x = X.T.astype(np.float64)
            gap = worst = 0.0
            for k in range(K):
                Psi = post["U"][k] @ post["U"][k].T
                args = (post["kappa"][k], post["nu"][k], post["m"][k], Psi)
                cen = B.update_centred(*args, W[:, k], x)
                unc = B.update_uncentred(*args, W[:, k].sum(), W[:, k] @ x, (W[:, k, None] * x).T @ x)
                gap = max(gap, B.rel(unc[3], cen[3]), B.rel(unc[2], cen[2]))
                U1 = p.post["U"][k]
                worst = max(worst, B.rel(U1 @ U1.T, cen[3]), B.rel(p.post["m"][k], cen[2]), abs(p.post["kappa"][k] - cen[0]) / cen[0],
                            abs(p.post["nu"][k] - cen[1]) / cen[1])
            print(mode, "formulation gap", gap, "absorbed posterior at", worst / (8 * gap), "of the tolerance")
            assert worst <= 8 * gap
            assert np.allclose(p.points_count, counts + got.N, rtol=1e-15) and abs(p.points_count.sum() - counts.sum() - n) <= n * K * 2.0 ** -23
            after = p.predict(Y)
            assert not same(before[1], after[1])                                                     # the model moved
            with open_predictor(host, p.post, 256, counts=p.points_count) as fresh:                  # ... to exactly the absorbed posterior:
                want = fresh.predict(Y)                                                              # the worker was really reloaded
            assert same(after[0], want[0]) and same(after[1], want[1])
            path = str(tmp_path / f"{mode}.npz")
            p.save(path)
            snap = {k: v.copy() for k, v in p.post.items()}
            none = p.absorb(np.full((D, 300), np.nan, np.float32), assign=mode)                      # all skipped: no bit changes
            assert none.skipped == 300 and none.N.sum() == 0 and all(same(p.post[k], snap[k]) for k in snap)
            again = p.predict(Y)
            assert same(again[0], after[0]) and same(again[1], after[1])
        with host.Predictor.load(path, capacity=64) as q:
            loaded = q.predict(Y)
            assert all(same(q.post[k], snap[k]) for k in snap)
        assert same(loaded[0], after[0]) and same(loaded[1], after[1])


# ------------------------------------------------------------------------------------------------ calls
def test_refusals_come_before_any_launch(pkg):
    n = 300
    rng = np.random.default_rng(3)
    wk = pkg.Worker(pkg.PRIOR_NIW, 2, n, device=0, seed=1)
    wk.upload_points(rng.standard_normal((n, 2)).astype(np.float32))

    def refused(code, fn, *a, what=(), **kw):
        with pytest.raises(pkg.DpmmError) as e:
            fn(*a, **kw)
        assert e.value.code == code, str(e.value)
        for w in what:
            assert w in str(e.value), str(e.value)

    refused(-4, wk.batchstats_begin)                                    # DPMM_ESTATE: no predictive parameters yet
    refused(-4, wk.batchstats_accumulate, n)                            # no dpmm_batchstats_begin
    refused(-4, wk.batchstats_read_raw)
    with pytest.raises((RuntimeError, pkg.DpmmError)):
        wk.batchstats_read()
    wk.set_predictive_niw(*S.niw_params(rng, 2, 3))
    refused(-4, wk.batchstats_accumulate, n)                            # a refused begin starts nothing
    refused(-1, wk.batchstats_begin, 2, what=("mode",))
    wk.batchstats_begin(1, -50.0)
    refused(-1, wk.batchstats_accumulate, n + 1, what=("n_valid",))
    refused(-1, wk.batchstats_accumulate, -1, what=("n_valid",))
    assert wk._lib.dpmm_batchstats_read(wk._h, None) == -1              # out == NULL
    wk.batchstats_accumulate(n)
    wk.batchstats_accumulate(0)                                         # nothing
    got = wk.batchstats_read()
    assert got["count"].sum() + got["held_out"][0] == n and got["skipped"][0] == 0 and got["incomplete"][0] == 0
    wk.set_predictive_niw(*S.niw_params(rng, 2, 4))                    # another K than begin saw
    refused(-4, wk.batchstats_accumulate, n, what=("changed",))
    wk.batchstats_begin(0)
    wk.set_predictive_niw(*S.niw_params(rng, 2, 4))                    # the same K, other parameters
    refused(-4, wk.batchstats_accumulate, n, what=("changed",))
    r = wk.batchstats_read()
    assert r["count"].sum() == 0 and not r["S"].any()                   # nothing was launched: the accumulators are as begin left them
    wk.close()
    mult = pkg.Worker(pkg.PRIOR_MULT, 8, n, device=0, seed=1)
    refused(-1, mult.batchstats_begin, what=("Multinomial",))           # DPMM_EINVAL, whatever its state
    mult.close()
