"""CPU-side checks of the marginal typicality and explanation of points with gaps (DPMM_OPT_TYPICALITY_GAPS): the reference of
tests/test_gpu_gap_typicality.py (tests/tools/gap_typicality_ref.py) against identities it does not use, the option number in the header
and the binding, and the `gaps=` keyword's refusals, which come before the worker is touched."""
import importlib
import os
import re

import numpy as np
import pytest

import test_missing_cpu as MC
from __graft_entry__ import ROOT, load_package
from tools import explain_ref as E
from tools import gap_typicality_ref as G
from tools import sample_ref as SR
from tools import typicality_ref as T

HEADER = os.path.join(ROOT, "include", "dpmm_hip_typicality.h")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


def case(D, r, seed, n=12):
    """(X with r gaps per point, lab0, params): K = 2, the gap positions random per point."""
    rng = np.random.default_rng(seed)
    post, m, A, df = SR.niw_model(D, 2, D + 3.0, seed)
    lab0 = rng.integers(0, 2, n)
    x = m[lab0] + 2.0 * np.einsum("nij,nj->ni", A[lab0], rng.standard_normal((n, D)))
    X = x.T.astype(np.float32)
    for i in range(n):
        X[rng.choice(D, r, replace=False), i] = np.nan
    R = np.linalg.inv(A)                                                 # upper triangular, R'R = (A A')^-1
    return X, lab0, T.worker_params(m, R, df)


@pytest.mark.parametrize("D,r", [(2, 1), (5, 1), (5, 4), (9, 3), (20, 16), (70, 2)])
def test_reference_against_independent_identities(D, r):
    X, lab0, (m, R, df) = case(D, r, 100 * D + r)
    ref = G.reference(X, lab0, m, R, df)
    for i in range(X.shape[1]):
        k = lab0[i]
        Rk, mk, dfk = R[k].astype(np.float64), m[k].astype(np.float64), float(df[k])
        mis, obs = np.flatnonzero(np.isnan(X[:, i])), np.flatnonzero(~np.isnan(X[:, i]))
        z = np.zeros(D)
        z[obs] = X[obs, i].astype(np.float64) - mk[obs]
        # q_o is the least q over the missing features, attained at the conditional mean m_M - t
        y, C = Rk @ z, Rk[:, mis]
        t = np.linalg.solve(C.T @ C, C.T @ y)
        res = y - C @ t
        assert abs(res @ res - ref.q[i]) <= 1e-9 * (1 + ref.q[i])
        zf = z.copy()
        zf[mis] = -t                                                     # x_M = m_M - t
        assert abs(np.sum((Rk @ zf) ** 2) - ref.q[i]) <= 1e-9 * (1 + ref.q[i])
        for _ in range(3):
            zp = zf.copy()
            zp[mis] += np.random.default_rng(i).standard_normal(r)
            assert np.sum((Rk @ zp) ** 2) >= ref.q[i] * (1 - 1e-12)
        # R' res vanishes on M and is g' on O
        g = Rk.T @ res
        assert np.abs(g[mis]).max() <= 1e-9 * (1 + np.abs(g).max())
        assert np.allclose(g[obs], ref.gprime[i, obs], rtol=1e-8, atol=1e-10)
        # a'_d = 1 / (variance scale of feature d given the other observed ones), by a brute-force Schur complement of Sigma
        S = np.linalg.inv(Rk.T @ Rk)
        for d in obs[:4]:
            rest = np.array([j for j in obs if j != d], np.int64)
            var = S[d, d] - (S[d, rest] @ np.linalg.solve(S[np.ix_(rest, rest)], S[rest, d]) if len(rest) else 0.0)
            assert abs(ref.aprime[i, d] * var - 1) <= 1e-8
        # the z-scores by the textbook route on the observed features alone
        Ro, _ = G.marginal_factor(Rk, obs)
        want = E.direct_conditional(X[obs, i], mk[obs], Ro, dfk)
        assert np.allclose(ref.t[i, obs], want, rtol=1e-7, atol=1e-9)
        assert np.isnan(ref.t[i, mis]).all() and np.isnan(ref.e[i, mis]).all() and np.isnan(ref.ftail[i, mis]).all()
        assert np.all(ref.e_bound[i, obs] > 0) and np.all(ref.t_bound[i, obs] > 0) and ref.q_bound[i] > 0
    assert np.allclose(ref.tail, T.tail_of(ref.q, df.astype(np.float64)[lab0], D - r), rtol=1e-12)


def test_one_observed_feature_collapses():
    """D_o = 1: zscore^2 = q_o and feature_tail = tail."""
    X, lab0, (m, R, df) = case(5, 4, 77)
    ref = G.reference(X, lab0, m, R, df)
    obs = ~np.isnan(X.T)
    assert np.allclose(ref.t[obs] ** 2, ref.q, rtol=1e-10) and np.allclose(ref.ftail[obs], ref.tail, rtol=1e-9)


def test_option_number_in_header_and_binding(pkg):
    binding = importlib.import_module(pkg.__name__ + ".binding")
    hdr = open(HEADER).read()
    assert int(re.search(r"#define DPMM_OPT_TYPICALITY_GAPS (\d+)", hdr).group(1)) == binding.OPT_TYPICALITY_GAPS == 35
    for h in os.listdir(os.path.join(ROOT, "include")):                  # the key is free: no other header gives 35 to an option
        src = open(os.path.join(ROOT, "include", h)).read()
        keys = re.findall(r"\b(DPMM_OPT_[A-Z0-9_]+)\s*=?\s+(\d+)\s*[,/\n]", src)
        assert [k for k, v in keys if int(v) == binding.OPT_TYPICALITY_GAPS and k != "DPMM_OPT_TYPICALITY_GAPS"] == [], h


def test_the_keyword_refuses_before_the_worker_is_touched(score, pkg):
    binding = importlib.import_module(pkg.__name__ + ".binding")
    D, K = 3, 4
    X = MC.gappy(D, 37)
    for kw in (dict(), dict(missing="propagate")):
        with score.Predictor(MC.model(0, D, K), capacity=10, worker_factory=MC.StandIn, **kw) as p:
            for call in (lambda: p.typicality(X, gaps="marginalize"), lambda: p.explain(X, gaps="marginalize"),
                         lambda: p.explain(X, top=2, gaps="marginalize")):
                with pytest.raises(ValueError, match='missing="marginalize"'):
                    call()
            with pytest.raises(ValueError, match="gaps must be"):
                p.typicality(X, gaps="impute")
            assert p._wk.options == [] and p._wk.uploads == 0
    with score.Predictor(MC.model(1, D, K), capacity=10, worker_factory=MC.StandIn) as p:      # Multinomial
        for call in (lambda: p.typicality(X, gaps="marginalize"), lambda: p.explain(X, gaps="marginalize")):
            with pytest.raises(ValueError):
                call()
        assert p._wk.options == [] and p._wk.uploads == 0
    with pytest.raises(ValueError, match='missing="marginalize"'):       # the one-shots pass the keyword on
        score.typicality(MC.model(0, D, K), X, gaps="marginalize", worker_factory=MC.StandIn)
    with pytest.raises(ValueError, match='missing="marginalize"'):
        score.explain(MC.model(0, D, K), X, top=2, gaps="marginalize", worker_factory=MC.StandIn)
    with score.Predictor(MC.model(0, D, K), capacity=10, worker_factory=MC.StandIn, missing="marginalize") as p:
        assert p._gaps_option("marginalize", "typicality") == 1 and p._gaps_option("incomplete", "typicality") == 0
        assert p._wk.options == [(binding.OPT_SCORE_MISSING, 1)]
