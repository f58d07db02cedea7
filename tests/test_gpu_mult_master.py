"""The Multinomial device master (csrc/mult_master.hip) by VALUE: the Dirichlet draws, the log-marginals and the hand-over images against
the Float64 restatement tests/tools/mult_master_ref.py on the inputs of tests/tools/mult_master_cases.py (rows fed through
dpmm_mult_master_put_rows, so every count regime is reached without data).

Tolerances.  Draws: one Float32 ulp (np.spacing of the reference value) on every entry -- both sides round the same Float64 quantity to
Float32, device and numpy log / cos / sqrt / exp differ by a few Float64 ulp, and tests/test_mult_master_ref_cpu.py asserts on these very
inputs that no decisive comparison is within 1e-9 of flipping and that no entry loses its Float32 digits to the difference lg - lse.
Log-marginals: N equal; L to rtol 1e-10 (the figure of the host comparison in test_gpu_mult.py) + 8 * 2^-53 * (|lgamma(sum a')| +
sum |lgamma(a'_d)|), the rounding of the terms that are summed.  Hand-over: bit-equal tables and equal labels between the images packed
behind a device draw and those packed from the same values given by the host."""
import importlib

import numpy as np
import pytest

from tools import mult_master_cases as C
from tools import mult_master_ref as M

pytestmark = pytest.mark.gpu
ELIMIT = -5


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def binding(pkg):
    return importlib.import_module("dpmmsubclusters_jl_amd.binding")


def rows_worker(pkg, D, seed, alpha, alpha_outlier=None):
    """A worker that is given rows, not data: a handful of zero points stand in for the shard."""
    wk = pkg.Worker(pkg.PRIOR_MULT, D, 4, device=0, seed=seed)
    wk.upload_points(np.zeros((4, D), np.float32))
    wk.mult_master_setup(alpha, alpha_outlier)
    return wk


def weights(K, seed=0):
    rng = np.random.default_rng(seed)
    return rng.dirichlet(np.full(2, 5.0), size=K).astype(np.float32), rng.dirichlet(np.full(K, 5.0)).astype(np.float32)


def logsumexp_rows(lp):
    lp = lp.astype(np.float64)
    m = lp.max(1)
    return m + np.log(np.exp(lp - m[:, None]).sum(1))


def assert_draws(got, want, what):
    ulp = M.ulp_distance(got, want)
    share = float((got == want).mean())
    print(f"\nMULT_MASTER draws {what}: max ulp distance {ulp.max():.3g}, bit-equal share {share:.6f} of {got.size}")
    j, d = np.unravel_index(int(ulp.argmax()), ulp.shape)
    assert ulp.max() <= 1.0, f"{what}: row {j} feature {d}: device {got[j, d]!r} reference {want[j, d]!r} ({ulp.max():.3g} ulp); bit-equal share {share:.6f}"
    assert np.all(np.abs(logsumexp_rows(got)) <= 1e-5), what


# ------------------------------------------------------------------------------------------------ draws
@pytest.mark.parametrize("case", C.draw_cases(), ids=repr)
def test_draws_by_value(pkg, case):
    """mult_dirichlet_kernel: every entry of every row set within one Float32 ulp of the reference; rows normalised; another epoch gives
    other draws, the same epoch the same.  Outlier cases: rows 0..2 follow alpha_outlier under outlier_first and nothing does without."""
    K = case.K
    wk = rows_worker(pkg, case.D, case.seed, case.alpha, case.alpha_outlier)
    lr, w = weights(K)
    follows = 0.0                                         # the largest share, over the row sets, of entries of rows 0..2 that left the cluster prior
    for v, rows in enumerate(case.rows):
        wk.mult_master_put_rows(rows)
        wk.mult_master_draw(case.epoch, lr, w, case.outlier_first)
        a = wk.mult_master_draws(K)
        wk.mult_master_draw(case.epoch + 1, lr, w, case.outlier_first)
        b = wk.mult_master_draws(K)
        wk.mult_master_draw(case.epoch, lr, w, case.outlier_first)
        c = wk.mult_master_draws(K)
        want, _, _ = M.dirichlet_logp(rows, case.alpha, case.alpha_outlier, case.outlier_first, case.seed, case.epoch)
        assert_draws(a, want, f"{case!r} rows {v}")
        assert np.array_equal(a, c)
        if case.D > 1:                                   # (D = 1: log p = 0 whatever the variate)
            assert not np.array_equal(a, b) and not np.array_equal(a[0], a[min(3, 3 * K - 1)])
        if case.outlier == "first":
            other, _, _ = M.dirichlet_logp(rows, case.alpha, None, False, case.seed, case.epoch)
            follows = max(follows, float((M.ulp_distance(a[:3], other[:3]) > 1.0).mean()))
            assert M.ulp_distance(a[3:], other[3:]).max() <= 1.0
    assert case.outlier != "first" or follows > 0.9       # (a populated cluster 0 hardly feels its prior; the empty one is the prior)
    wk.close()


def test_outlier_first_needs_an_outlier_prior(pkg):
    case = C.Case(300, 4, "mixed", "unused")               # (a case of the list: its values do not depend on the outlier prior)
    wk = rows_worker(pkg, case.D, case.seed, case.alpha)
    wk.mult_master_put_rows(case.rows[0])
    lr, w = weights(case.K)
    with pytest.raises(pkg.DpmmError):
        wk.mult_master_draw(case.epoch, lr, w, True)
    wk.mult_master_pairs_ahead([0], [1], outlier_first=True)
    with pytest.raises(pkg.DpmmError):
        wk.mult_master_marginals(case.K)
    wk.mult_master_draw(case.epoch, lr, w, False)          # (and the refusals left the worker usable)
    want, _, _ = M.dirichlet_logp(case.rows[0], case.alpha, None, False, case.seed, case.epoch)
    assert_draws(wk.mult_master_draws(case.K), want, "after the refusal")
    wk.close()


def test_limits_of_the_feature_dimension(pkg):
    """DPMM_MULT_MASTER_MAXD = 16384: one more is refused at setup (DPMM_ELIMIT); 16384 itself -- 128 KB of dynamic LDS, an attribute the
    launcher sets once per process -- draws after a draw at a small D in the same process."""
    wk = pkg.Worker(pkg.PRIOR_MULT, C.MAXD + 1, 4, device=0, seed=1)
    with pytest.raises(pkg.DpmmError) as e:
        wk.mult_master_setup(np.ones(C.MAXD + 1, np.float32))
    assert e.value.code == ELIMIT
    wk.close()
    for D in (2, C.MAXD, 255):
        case = C.Case(D, 2, "ones")
        wk = rows_worker(pkg, D, case.seed, case.alpha)
        wk.mult_master_put_rows(case.rows[0])
        wk.mult_master_draw(case.epoch, *weights(2))
        want, _, _ = M.dirichlet_logp(case.rows[0], case.alpha, None, False, case.seed, case.epoch)
        assert_draws(wk.mult_master_draws(2), want, f"D = {D} in one process")
        wk.close()


# ------------------------------------------------------------------------------------------------ log-marginals
def assert_marginals(got, want, scale, what):
    atol = 8 * 2.0 ** -53 * scale
    err = np.abs(got - want)
    rel = float(np.max(err / np.maximum(np.abs(want), 1.0), initial=0.0))          # (relative to max(|L|, 1): L = 0 for empty rows and for D = 1)
    used = float(np.max(np.where(err == 0.0, 0.0, err / np.maximum(1e-10 * np.abs(want) + atol, np.finfo(np.float64).tiny)), initial=0.0))
    print(f"\nMULT_MASTER marginals {what}: max relative error {rel:.3g}, {used:.3g} of the tolerance, absolute term up to {float(np.max(atol, initial=0.0)):.3g}")
    assert np.all(err <= 1e-10 * np.abs(want) + atol), f"{what}: max relative error {rel:.3g}, {used:.3g} of the tolerance"


def marginals_of(wk, case, rows, pairs, outlier_first):
    wk.mult_master_put_rows(rows)                        # (new rows: nothing answered before is valid)
    wk.mult_master_pairs_ahead(pairs[:, 0], pairs[:, 1], outlier_first=outlier_first)
    return wk.mult_master_marginals(case.K)


@pytest.mark.parametrize("case", C.marginal_cases(), ids=repr)
def test_marginals_by_value(pkg, case):
    """mult_marginal_kernel: N equal, L and the pooled L of every ordered pair of the 8 clusters -- all C(8, 2), (0, j) and (j, 0), i = j --
    with the outlier prior unused and followed by cluster 0 (a pair takes the prior of its first index)."""
    wk = rows_worker(pkg, case.D, case.seed, case.alpha, case.alpha_outlier)
    pairs = C.all_pairs(case.K)
    for outlier_first in (False, True):
        N, L, P = marginals_of(wk, case, case.rows[0], pairs, outlier_first)
        wN, wL, wP, sL, sP = M.log_marginals(case.rows[0], case.alpha, case.alpha_outlier, outlier_first, pairs)
        assert np.array_equal(N, wN) and len(P) == len(pairs)
        assert_marginals(L, wL, sL, f"{case!r} outlier_first={outlier_first} rows")
        assert_marginals(P, wP, sP, f"{case!r} outlier_first={outlier_first} pairs")
        assert np.all(L[wN == 0] == 0.0)
    wk.close()


def test_limits_of_the_pair_list(pkg):
    """Exactly DPMM_MULT_MASTER_MAXPAIRS = 8192 pairs are answered; 8193, or an index >= K, leave the rows answered and no pair."""
    case = C.Case(257, C.MARGINAL_K, "mixed", "first")
    wk = rows_worker(pkg, case.D, case.seed, case.alpha, case.alpha_outlier)
    rng = np.random.default_rng(5)
    pairs = rng.integers(0, case.K, (C.MAXPAIRS + 1, 2)).astype(np.int32)
    wN, wL, wP, sL, sP = M.log_marginals(case.rows[0], case.alpha, case.alpha_outlier, True, pairs)
    N, L, P = marginals_of(wk, case, case.rows[0], pairs[:C.MAXPAIRS], True)
    assert len(P) == C.MAXPAIRS and np.array_equal(N, wN)
    assert_marginals(P, wP[:C.MAXPAIRS], sP[:C.MAXPAIRS], "8192 pairs")
    bad = pairs[:5].copy()
    bad[3, 1] = case.K
    for what, pp in (("8193 pairs", pairs), ("an index >= K", bad)):
        N, L, P = marginals_of(wk, case, case.rows[0], pp, True)
        assert len(P) == 0 and np.array_equal(N, wN), what
        assert_marginals(L, wL, sL, what)
    N, L, P = marginals_of(wk, case, case.rows[0], pairs[:3], True)           # (and a good list is answered again)
    assert_marginals(P, wP[:3], sP[:3], "3 pairs after the refused lists")
    wk.close()


def test_marginals_refuse_a_partial_pass(pkg):
    D, n, K = 130, 64, 2
    wk = pkg.Worker(pkg.PRIOR_MULT, D, n, device=0, seed=3)
    wk.upload_points(np.ones((n, D), np.float32))
    wk.set_labels(1 + np.arange(n) % K, 1 + (np.arange(n) // K) % 2)
    wk.set_num_clusters(K)
    wk.mult_master_setup(np.ones(D, np.float32))
    wk.suffstats_packed(None)
    N, L, P = wk.mult_master_marginals(K)
    assert N.tolist() == [32, 16, 16, 32, 16, 16] and len(P) == 0
    wk.suffstats_packed(np.array([1]))
    with pytest.raises(pkg.DpmmError):
        wk.mult_master_marginals(K)
    wk.close()


# ------------------------------------------------------------------------------------------------ hand-over
def to_csc(X):
    r, c = np.nonzero(X)
    colptr = np.zeros(X.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=X.shape[0]), out=colptr[1:])
    return colptr, c.astype(np.int64), X[r, c].astype(np.float32)


HANDOVER = [(kind, D) for kind in ("bytes", "bf16", "f32") for D in (127, 128, 129, 300)] + [("csc", 300)]


@pytest.mark.parametrize("kind,D", HANDOVER)
def test_handover_images_of_a_device_draw(pkg, kind, D):
    """The images the sweep kernels read (byte planes, bf16 planes, Float32 fragments, the sparse image) packed behind a device draw are
    the ones packed from the same log-probabilities and weights given through dpmm_set_params_mult: bit-equal tables, equal labels and
    sub-labels of one sweep (the sub-cluster rows 3k+1, 3k+2 do not show in the table), and the table is x . logp + log w."""
    n, K, seed, epoch = 2049, 5, 41, 9
    rng = np.random.default_rng([D, len(kind)])
    X = rng.poisson(0.6, (n, D)).astype(np.float32)
    X[::7, 0] = 255.0
    if kind == "bf16":
        X = X * 2.0                                       # integers, some above 255, eight significant bits
        assert X.max() > 255
    elif kind == "f32":
        X = (X + rng.random(X.shape).astype(np.float32) * np.float32(0.37)).astype(np.float32)
    lab0, sub0 = 1 + rng.integers(0, K, n), 1 + rng.integers(0, 2, n)
    alpha = rng.uniform(0.15, 2.5, D).astype(np.float32)
    lr, w = weights(K, seed=D)
    wk = pkg.Worker(pkg.PRIOR_MULT, D, n, first_index=77, device=0, seed=seed)
    wk.upload_points_csc(*to_csc(X)) if kind == "csc" else wk.upload_points(X)
    wk.mult_master_setup(alpha)
    res = []
    for source in ("device", "host"):
        wk.set_labels(lab0, sub0)
        wk.set_num_clusters(K)
        rows = wk.suffstats_packed(None)
        if source == "device":
            wk.mult_master_draw(epoch, lr, w)
            logp = wk.mult_master_draws(K)
            assert rows[:, 0].min() > 0 and np.all(np.abs(logsumexp_rows(logp)) <= 1e-5)
        else:
            wk.set_params_mult(logp, lr, w)
        tab = wk.debug_loglik()
        wk.sweep(epoch)
        res.append((tab, *wk.get_labels()))
    wk.close()
    assert np.array_equal(res[0][0], res[1][0])
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
    assert len(np.unique(res[0][1])) > 1 and len(np.unique(res[0][2])) == 2
    want = np.stack([X.astype(np.float64) @ logp[3 * k].astype(np.float64) + np.log(np.float64(w[k])) for k in range(K)])
    np.testing.assert_allclose(res[0][0], want, rtol=1e-5, atol=1e-3)


# ------------------------------------------------------------------------------------------------ draws launched ahead
@pytest.mark.parametrize("D", C.AHEAD_DIMS)
def test_draws_launched_ahead_by_value(pkg, binding, D):
    """DPMM_OPT_MULT_DRAWS_AHEAD: the draws dpmm_step_stats launches behind the statistics are taken by the guessed dpmm_mult_master_draw
    (the counter says so) and are the reference values; another epoch, or the other outlier flag, falls back to a draw inside the call --
    the reference values too."""
    a = C.AheadCase(D)
    K = a.K
    wk = pkg.Worker(pkg.PRIOR_MULT, D, a.n, device=0, seed=a.seed)
    wk.set_option(binding.OPT_MULT_DRAWS_AHEAD, 1)
    wk.upload_points(a.X)
    wk.set_labels(a.labels, a.sub)
    wk.set_num_clusters(K)
    wk.mult_master_setup(a.alpha, a.alpha_outlier)
    assert np.array_equal(wk.suffstats_packed(None)[:, :1 + D], a.rows)
    lr, w = weights(K)
    wk.mult_master_draw(a.epoch0, lr, w)
    none = np.zeros(0, np.int32)
    taken = [True, False, False]
    for (epoch, outlier_first), ahead in zip(a.draws, taken):
        used = wk.debug_mult_draws_ahead()
        wk.mult_master_pairs_ahead(none, none, outlier_first=False)
        packed, bad = wk.step_stats(1)
        assert np.array_equal(packed[:, :1 + D], a.rows) and not bad.any()
        wk.mult_master_draw(epoch, lr, w, outlier_first)
        assert wk.debug_mult_draws_ahead() == used + int(ahead), (epoch, outlier_first)
        want, _, _ = M.dirichlet_logp(a.rows, a.alpha, a.alpha_outlier, outlier_first, a.seed, epoch)
        assert_draws(wk.mult_master_draws(K), want, f"{a!r} epoch {epoch} outlier_first={outlier_first} ahead={ahead}")
    wk.close()
