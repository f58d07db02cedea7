"""CPU-side checks of conditioning a fitted NIW mixture on a fixed set of features (host/condition.py, include/dpmm_hip_regress.h): the
closure rule, the regression tables, the reference of tests/test_gpu_regress.py itself -- a second independent form, planted mistakes outside
the bound -- the refusals, and the C boundary.  Float64, no GPU."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from __graft_entry__ import load_package
from fake_worker import FakeWorker
from tools import predictive_ref as pr
from tools import regress_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dpmm_hip_regress.h")
FUNCS = ["dpmm_regress_points", "dpmm_regress_points_device", "dpmm_set_regression"]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


@pytest.fixture(scope="module")
def cond(pkg):
    return importlib.import_module(pkg.__name__ + ".host.condition")


@pytest.fixture(scope="module")
def priors(pkg):
    return importlib.import_module(pkg.__name__ + ".host.priors")


def random_posterior(D, K, seed):
    """Well-conditioned posteriors: cond(Psi) <= 1e4 (singular values of U in 1 .. 100)."""
    rng = np.random.default_rng(seed)
    U = np.empty((K, D, D))
    for k in range(K):
        Q1, _ = np.linalg.qr(rng.standard_normal((D, D)))
        Q2, _ = np.linalg.qr(rng.standard_normal((D, D)))
        G = (Q1 * np.geomspace(1.0, 100.0, D)) @ Q2
        Psi = G @ G.T
        U[k] = np.linalg.cholesky(Psi[::-1, ::-1])[::-1, ::-1]
        assert np.allclose(U[k] @ U[k].T, Psi, rtol=1e-10) and np.allclose(U[k], np.triu(U[k])) and np.linalg.cond(Psi) <= 1.0001e4
    nu = D + rng.uniform(1.0, 30.0, K)
    return dict(kappa=rng.uniform(0.5, 20.0, K), nu=nu, m=rng.standard_normal((K, D)), U=U,
                logdet_psi=np.array([np.linalg.slogdet(U[k] @ U[k].T)[1] for k in range(K)]) - D * np.log(nu))


def predictive(priors, post, D, w):
    out = {}

    class Cap:
        def predict_table_niw(self, m, R, logdet, df, weights, points=False):
            out["args"] = tuple(np.asarray(a, np.float64) for a in (m, R, logdet, df, weights))
    priors.niw_hyperparams(1.0, np.zeros(D), D + 3.0, np.eye(D)).predictive_table(Cap(), post, list(range(len(w))), w)
    m, R, logdet, df, w = out["args"]
    return m, R.reshape(len(w), D, D), logdet, df, w


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


@pytest.mark.parametrize("D", [3, 8, 65])
def test_closure_against_the_dense_form(cond, priors, D):
    K = 3
    post = random_posterior(D, K, D)
    w = np.array([0.2, 0.3, 0.5])
    m, R, logdet, df, _ = predictive(priors, post, D, w)
    rng = np.random.default_rng(D + 1)
    for Do in sorted({1, D // 2, D - 1}):
        O = rng.permutation(D)[:Do]                                # scrambled order
        sub = cond.niw_marginal(post, O)
        assert np.allclose(sub["U"], np.triu(sub["U"])) and sub["U"].shape == (K, Do, Do)
        mo, Ro, ldo, dfo, _ = predictive(priors, sub, Do, w)
        assert np.array_equal(dfo, df)                             # the same degrees of freedom, exactly
        for k in range(K):
            S = np.linalg.inv(R[k].T @ R[k])[np.ix_(O, O)]
            assert np.array_equal(mo[k], m[k, O])
            assert rel(np.linalg.inv(Ro[k].T @ Ro[k]), S) <= 1e-10
            assert abs(ldo[k] - np.linalg.slogdet(S)[1]) <= 1e-10 * max(1.0, abs(ldo[k]))
            # logdet_psi as posterior() defines it: that of Psi[O, O] / nu'
            Psi = (post["U"][k] @ post["U"][k].T)[np.ix_(O, O)]
            assert abs(sub["logdet_psi"][k] - (np.linalg.slogdet(Psi)[1] - Do * np.log(sub["nu"][k]))) <= 1e-10 * max(1.0, abs(sub["logdet_psi"][k]))
            assert sub["nu"][k] == post["nu"][k] - (D - Do) and sub["kappa"][k] == post["kappa"][k]


def test_hyper_parameters_follow_the_same_rule(cond):
    D, O = 6, [4, 0, 3]
    rng = np.random.default_rng(0)
    G = rng.standard_normal((D, D))
    hyper = dict(kappa=2.0, m=rng.standard_normal(D), nu=D + 4.0, psi=G @ G.T + D * np.eye(D))
    sub = cond.hyper_marginal(hyper, O)
    assert sub["nu"] == hyper["nu"] - 3 and sub["kappa"] == 2.0 and np.array_equal(sub["m"], hyper["m"][O])
    assert np.allclose(sub["nu"] * sub["psi"], hyper["nu"] * hyper["psi"][np.ix_(O, O)], rtol=1e-14)


@pytest.mark.parametrize("D", [3, 8, 65])
def test_regression_tables_against_the_dense_inverse(cond, priors, D):
    K = 3
    post = random_posterior(D, K, 10 + D)
    w = np.array([0.5, 0.3, 0.2])
    m, R, logdet, df, _ = predictive(priors, post, D, w)
    rng = np.random.default_rng(D)
    perm = rng.permutation(D)
    for Do, Dt in ((1, D - 1), (D - 1, 1), (D // 2, D - D // 2), (1, 1)):       # the last: features in neither set are marginalised away
        O, M = perm[:Do], perm[Do:Do + Dt]
        B, c, V = cond.regression_tables(m, R, O, M)
        for k in range(K):
            S = np.linalg.inv(R[k].T @ R[k])
            G = S[np.ix_(M, O)] @ np.linalg.inv(S[np.ix_(O, O)])
            assert rel(B[k], G) <= 1e-9 and rel(c[k], m[k, M] - G @ m[k, O]) <= 1e-9
            assert rel(V[k], np.diag(S[np.ix_(M, M)] - G @ S[np.ix_(O, M)])) <= 1e-9
        # h reproduces the marginal Student-t log-density + log w at three points
        sub = cond.niw_marginal(post, O)
        mo, Ro, ldo, dfo, _ = predictive(priors, sub, Do, w)
        h = cond.table_constant(ldo, dfo, w, Do)
        x = rng.standard_normal((3, Do)) * 3
        want = rr.marginal_logdens(post, w, O, x)
        got = h[None, :] - 0.5 * (dfo + Do)[None, :] * np.log1p(rr.quad(x, mo, Ro) / dfo[None, :])
        assert np.max(np.abs(got - want)) <= 1e-9 * np.max(np.abs(want))
        try:
            from scipy.stats import multivariate_t
        except ImportError:
            continue
        for k in range(K):
            S = np.linalg.inv(R[k].T @ R[k])[np.ix_(O, O)]
            assert np.allclose(multivariate_t(loc=m[k, O], shape=S, df=df[k]).logpdf(x) + np.log(w[k]), got[:, k], rtol=1e-9, atol=1e-9)


def reference_inputs(cond, priors, Do, Dt, K):
    c = rr.make_case(Do, Dt, K)
    D = c["D"]
    w = rr.weights(10 + 5 * np.arange(K))
    m, R, logdet, df, _ = predictive(priors, c["post"], D, w)
    B, cc, V = cond.regression_tables(m, R, c["given"], c["targets"])
    sub = cond.niw_marginal(c["post"], c["given"])
    mo, Ro, ldo, dfo, _ = predictive(priors, sub, Do, w)
    x = c["X"].astype(np.float64)
    logp = rr.marginal_logdens(c["post"], w, c["given"], x)
    p = np.exp(logp - logp.max(1, keepdims=True))
    p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    return c, (m, R, df), (B, cc, V), (mo, Ro, dfo), x, p


@pytest.mark.parametrize("Do,Dt,K", [(3, 2, 3), (16, 17, 3), (33, 31, 1)])
def test_reference_against_the_dense_form_and_planted_mistakes(cond, priors, Do, Dt, K):
    c, (m, R, df), (B, cc, V), (mo, Ro, dfo), x, p = reference_inputs(cond, priors, Do, Dt, K)
    q = rr.quad(x, mo, Ro)
    ref = rr.reference(p, B, cc, V, dfo, q, x)
    mean2, std2 = rr.dense_form(p, m, R, df, c["given"], c["targets"], x)
    scale = np.abs(mean2).max()
    assert np.max(np.abs(ref["mean"] - mean2)) <= 1e-9 * scale
    # (the variance is a difference of squares of means up to 1e4 standard deviations out: compared at that scale)
    assert np.max(np.abs(ref["std"] ** 2 - std2 ** 2)) <= 1e-9 * max(scale * scale, 1.0)
    # the K = 1 closed form
    if K == 1:
        assert np.allclose(ref["std"], np.sqrt((dfo[0] + q[:, 0])[:, None] / (dfo[0] + Do - 2) * V[0][None, :]), rtol=1e-12)
    # ---- every planted mistake lands outside the bound, somewhere
    t = pr.error_bound(c["X"], mo.astype(np.float32), Ro.astype(np.float32), dfo.astype(np.float32),
                       pr.student_t_table(c["X"], mo, Ro, np.zeros(K), dfo, np.ones(K))[1]).T
    ref = rr.reference(p, B, cc, V, dfo, q, x, t=t)
    for mut in rr.MUTATIONS:
        if mut == "no_between_term" and K == 1:
            continue                                               # (one component: there is no between-component term)
        bad = rr.reference(p, B, cc, V, dfo, q, x, mutation=mut, D_full=c["D"], m_O=mo)
        out_mean = np.abs(bad["mean"] - ref["mean"]) > ref["mean_bound"]
        out_std = np.abs(bad["std"] - ref["std"]) > ref["std_bound"]
        assert (out_std.any() if mut in ("s_with_D", "no_between_term") else out_mean.any()), mut
    # ... and a restatement with Float32 tables and a Float32 chain lies inside it
    f = np.float32
    mu = cc.astype(f)[None, :, :].repeat(len(x), 0)
    for e in range(Do):
        mu = (mu.astype(np.float64) + B.astype(f)[None, :, :, e].astype(np.float64) * x[:, None, None, e]).astype(f)     # one rounding per step
    mean32 = (p.astype(np.float64)[:, :, None] * mu.astype(np.float64)).sum(1).astype(f)
    assert np.all(np.abs(mean32 - ref["mean"]) <= ref["mean_bound"])


class StandIn(FakeWorker):
    made = 0

    def __init__(self, *a, **kw):
        StandIn.made += 1
        super().__init__(*a, **kw)

    def set_predictive_niw(self, *a):
        pass

    def set_predictive_mult(self, *a):
        pass

    def set_option(self, *a):
        pass


def test_refusals_come_before_any_worker(score):
    import types
    D, K = 5, 2
    post, _ = rr.make_posterior(D, K, 1)
    with score.Predictor(rr.dummy_model(post, K, D), capacity=4, worker_factory=StandIn) as p:
        made = StandIn.made
        for bad in ([], [0, 0], [5], [-1], [0, 1, 2, 3, 4], [0.5], "ab"):
            with pytest.raises(ValueError):
                p.marginal(bad, worker_factory=StandIn)
            with pytest.raises(ValueError):
                p.regressor(bad, worker_factory=StandIn)
        with pytest.raises(ValueError, match="disjoint"):
            p.regressor([0, 1], [1, 2], worker_factory=StandIn)
        with pytest.raises(ValueError):
            p.regressor([0, 1], [], worker_factory=StandIn)
        p.projection = types.SimpleNamespace(D_in=9)
        with pytest.raises(ValueError, match="projection"):
            p.marginal([0, 1], worker_factory=StandIn)
        with pytest.raises(ValueError, match="projection"):
            p.regressor([0, 1], worker_factory=StandIn)
        p.projection = None
        assert StandIn.made == made
        with p.marginal([3, 1], worker_factory=StandIn) as mg:
            assert StandIn.made == made + 1 and mg.D == 2 and mg.K == K and mg.prior_hyper["m"].shape == (2,) and mg.missing == "propagate"
            assert np.array_equal(mg.post["m"], post["m"][:, [3, 1]]) and np.array_equal(mg.points_count, p.points_count)
    mult = types.SimpleNamespace(sampler=types.SimpleNamespace(K=2, prior=types.SimpleNamespace(kind=1, dim=4, alpha=np.ones(4)), post=dict(alpha=np.ones((6, 4), np.float32)),
                                                               alpha=1.0, points_count=np.ones(2), wk=types.SimpleNamespace(device=0)))
    with score.Predictor(mult, capacity=4, worker_factory=StandIn) as p:
        made = StandIn.made
        with pytest.raises(ValueError, match="NIW"):
            p.marginal([0, 1], worker_factory=StandIn)
        with pytest.raises(ValueError, match="NIW"):
            p.regressor([0, 1], worker_factory=StandIn)
        assert StandIn.made == made


# ------------------------------------------------------------------------------------------------ the C boundary
def test_header_compiles_as_c_and_is_bound_exported_and_built(pkg):
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER])
    hdr = open(HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", body))) == FUNCS
    binding = importlib.import_module(pkg.__name__ + ".binding")
    assert sorted(n for n, _, _ in binding.ABI_REGRESS) == FUNCS
    others = (binding.ABI + binding.ABI_TENSOR + binding.ABI_SCORE + binding.ABI_RANK + binding.ABI_OVERLAP + binding.ABI_BATCHSTATS + binding.ABI_TRACE
              + binding.ABI_MISSING + binding.ABI_IMPUTE + binding.ABI_CSC + binding.ABI_SAMPLE + binding.ABI_PROJECT)
    assert not set(FUNCS) & set(n for n, _, _ in others)
    assert int(re.search(r"#define DPMM_REGRESS_MAX_TARGETS (\d+)", hdr).group(1)) == binding.REGRESS_MAX_TARGETS == 256
    csrc = os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "build/regress.o" in re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "../../include/dpmm_hip_regress.h" in re.search(r"^build/dpmm_api\.o:(.*)$", mk, flags=re.M).group(1).split()
    hip = open(os.path.join(csrc, "regress.hip")).read()
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in hip and '#include "score_device.h"' in hip and not re.search(r"\batomic\w*\(", hip)
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for n in FUNCS:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                                   # additive: the version stays
    host = importlib.import_module(pkg.__name__ + ".host")
    for name in ("Regressor", "Regression", "regress"):
        assert getattr(host, name) is getattr(importlib.import_module(pkg.__name__ + ".host.score"), name)
    assert callable(binding.Worker.set_regression) and callable(binding.Worker.regress_points_into)
    assert host.Regression._fields == ("mean", "std", "labels", "skipped")
