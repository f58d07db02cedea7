"""CPU-side checks of the value-level reference of the Multinomial device master (tests/tools/mult_master_ref.py) on the inputs the GPU
tests use (tests/tools/mult_master_cases.py): the reference has the right law, every case is well conditioned (the 1-ulp comparison of
tests/test_gpu_mult_master.py rests on it), every mutant of the reference is told apart at the GPU tests' tolerances, and the
log-marginals agree with mpmath at 50 digits."""
import numpy as np
import pytest
from scipy.special import digamma, polygamma

from tools import mult_master_cases as C
from tools import mult_master_ref as M

MARGINAL_RTOL = 1e-10


@pytest.fixture(scope="module")
def references():
    """(case, [(logp, margin, headroom) per row set]) of every draw case, computed once"""
    out = []
    for case in C.draw_cases():
        out.append((case, [M.dirichlet_logp(rows, case.alpha, case.alpha_outlier, case.outlier_first, case.seed, case.epoch) for rows in case.rows]))
    return out


@pytest.mark.parametrize("a", [1e-3, 0.15, 1.0, 2.5, 1e4])
def test_law_of_the_reference_variates(a):
    """E log g = digamma(a), Var log g = trigamma(a): the mean of n = 20 000 variates to 5 standard errors (the a < 1 branch in logs: at
    a = 1e-3 the variates are near -1000 and a plain Gamma variate would underflow)."""
    n = 20000
    lg, margin = M.log_gamma_variates(np.full(n, a), seed=77, row=3, epoch=5)
    assert np.isfinite(lg).all() and margin > 0
    se = np.sqrt(polygamma(1, a) / n)
    assert abs(lg.mean() - digamma(a)) < 5 * se, (lg.mean(), digamma(a), se)
    # the same values one feature at a time and as rows of a matrix (the keying is by row and feature, not by call)
    one, _ = M.log_gamma_variates(np.full(7, a), seed=77, row=3, epoch=5)
    two, _ = M.log_gamma_variates(np.full((4, 7), a), seed=77, row=np.arange(4), epoch=5)
    assert np.array_equal(one, lg[:7]) and np.array_equal(two[3], lg[:7]) and not np.array_equal(two[2], lg[:7])


def test_every_case_is_well_conditioned(references):
    """A condition on the inputs, not a measurement: on every (seed, epoch, alpha, rows) the GPU test draws from, no decisive comparison of
    the rejection loop is closer than 1e-9 to flipping and no entry loses more than the headroom allows to the difference lg - lse."""
    for case, refs in references:
        margin, headroom = min(r[1] for r in refs), min(r[2] for r in refs)
        print(f"{case!r}: margin {margin:.3g} headroom {headroom:.3g}")
        assert margin >= C.MARGIN_MIN and headroom >= C.HEADROOM_MIN, (case, margin, headroom)
        for logp, _, _ in refs:
            assert logp.dtype == np.float32 and logp.shape == (3 * case.K, case.D) and np.isfinite(logp).all()
            assert np.allclose(np.exp(logp.astype(np.float64)).sum(1), 1.0, atol=1e-5)
    for D in C.AHEAD_DIMS:
        a = C.AheadCase(D)
        for epoch, outlier_first in a.draws:
            _, margin, headroom = M.dirichlet_logp(a.rows, a.alpha, a.alpha_outlier, outlier_first, a.seed, epoch)
            assert margin >= C.MARGIN_MIN and headroom >= C.HEADROOM_MIN, (a, epoch, margin, headroom)


def test_the_cases_cover_every_row_regime():
    for case in C.draw_cases() + C.marginal_cases():
        seen = set()
        for rows in case.rows:
            l, r = rows[0::2], rows[1::2]
            for k in range(case.K):
                nz = ((l[k, 1:] > 0).sum(), (r[k, 1:] > 0).sum())
                seen.add("empty" if l[k, 0] == 0 and r[k, 0] == 0 else "one-sided" if r[k, 0] == 0 else "populated")
                if rows[2 * k:2 * k + 2, 1:].max() == 1e7:
                    seen.add("1e7")
                if 1 in nz:
                    seen.add("single")
        assert seen == {"empty", "one-sided", "populated", "1e7", "single"}, (case, seen)


def _marginal_differs(case, mutate):
    pairs = C.all_pairs(case.K)
    for outlier_first in (False, True):
        _, L, P, sL, sP = M.log_marginals(case.rows[0], case.alpha, case.alpha_outlier, outlier_first, pairs)
        _, Lm, Pm, _, _ = M.log_marginals(case.rows[0], case.alpha, case.alpha_outlier, outlier_first, pairs, mutate=mutate)
        got, want, scale = np.concatenate([Lm, Pm]), np.concatenate([L, P]), np.concatenate([sL, sP])
        if np.any(np.abs(got - want) > MARGINAL_RTOL * np.abs(want) + 8 * 2.0 ** -53 * scale):
            return True
    return False


@pytest.mark.parametrize("mutate", M.MUTANTS)
def test_mutants_are_told_apart(references, mutate):
    """Every deliberately wrong reference differs from the true one by more than the GPU tests allow -- one Float32 ulp of a draw, or
    rtol 1e-10 + 8 * 2^-53 * scale of a log-marginal -- on at least one case: the GPU comparison would catch a kernel that made that
    mistake."""
    caught = []
    for case, refs in references:
        if case.D * case.K > 20000:                  # (the small cases suffice)
            continue
        for rows, (want, _, _) in zip(case.rows, refs):
            got, _, _ = M.dirichlet_logp(rows, case.alpha, case.alpha_outlier, case.outlier_first, case.seed, case.epoch, mutate=mutate)
            if M.ulp_distance(got, want).max() > 1.0:
                caught.append(repr(case))
                break
    for case in C.marginal_cases():
        if case.D <= 257 and _marginal_differs(case, mutate):
            caught.append("marginals " + repr(case))
    print(mutate, "caught on", len(caught), "cases:", caught[:6])
    assert caught, mutate


def test_log_marginals_against_mpmath():
    import mpmath as mp
    case = C.Case(7, 3, "mixed", "first")
    rows = case.rows[2]                              # cluster 0: empty; 1: single / small; 2: small / small
    rows[4, 1:] += np.array([1e7, 3, 0, 16777217.0, 0, 9_999_999, 1])          # big counts: Float32(sum) rounds
    pairs = C.all_pairs(3)
    with mp.workdps(50):
        def lm(prior, st):
            if st[0] == 0:
                return 0.0
            a = [mp.mpf(float(np.float32(p) + np.float32(s))) for p, s in zip(prior, st[1:])]
            pr = [mp.mpf(float(p)) for p in prior]
            return float(mp.loggamma(mp.fsum(pr)) - mp.loggamma(mp.fsum(a)) + mp.fsum(mp.loggamma(x) for x in a) - mp.fsum(mp.loggamma(x) for x in pr))
        for outlier_first in (False, True):
            N, L, P, sL, sP = M.log_marginals(rows, case.alpha, case.alpha_outlier, outlier_first, pairs)
            prior = lambda k: case.alpha_outlier if outlier_first and k == 0 else case.alpha
            want_L, want_N = [], []
            for k in range(3):
                l, r = rows[2 * k], rows[2 * k + 1]
                for st in (l + r, l, r):
                    want_L.append(lm(prior(k), st)); want_N.append(st[0])
            want_P = [lm(prior(i), rows[2 * i] + rows[2 * i + 1] + rows[2 * j] + rows[2 * j + 1]) for i, j in pairs.tolist()]
            assert np.array_equal(N, want_N)
            assert L[0] == L[1] == L[2] == 0.0 and P[0] == 0.0           # the empty cluster, and its pair with itself
            for got, want, scale in ((L, want_L, sL), (P, want_P, sP)):
                assert np.all(np.abs(got - np.array(want)) <= 1e-13 * np.abs(want) + 4 * 2.0 ** -53 * scale), (got, want)
