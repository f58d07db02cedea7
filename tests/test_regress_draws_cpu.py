"""CPU-side checks of the draws of the targets (include/dpmm_hip_regress_draw.h): the reference of tests/test_gpu_regress_draws.py itself -- its
two sides agree, every planted mistake is rejected by the comparison the GPU test makes, the law holds, the seeds the GPU tests use excuse
less than 1 % of the draws --, the factor W of host/condition.py, the argument checks, the Python walk over a stand-in worker and the C
boundary.  Float64, no GPU."""
import ctypes
import functools
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from __graft_entry__ import load_package
from fake_worker import FakeWorker
from tools import predictive_ref as pr
from tools import regress_draw_ref as rd
from tools import regress_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dpmm_hip_regress_draw.h")
FUNCS = ["dpmm_regress_draw_points", "dpmm_regress_draw_points_device", "dpmm_set_regression_factor"]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


@pytest.fixture(scope="module")
def cond(pkg):
    return importlib.import_module(pkg.__name__ + ".host.condition")


class StandIn(FakeWorker):
    """A worker that records its tables and `draws` a function of (global index, draw, target): what the walk has to put in place."""
    K_FAKE = 3
    OUT = 41          # the global index that takes no part

    def set_predictive_niw(self, *a):
        pass

    def set_option(self, *a):
        pass

    def set_regression(self, B, c, V, h):
        self.reg = (B, c, V, h)

    def set_regression_factor(self, W):
        self.W = np.array(W)

    def score_points_into(self, outs, m=0):
        outs["labels"][:] = 1 + (np.arange(len(outs["labels"])) % self.K_FAKE)

    def regress_draw_points_into(self, out, seed, i0, draw0=0, comp=None):
        n, nd, w = out.shape
        gi = i0 + np.arange(n)
        out[:] = (gi[:, None, None] * 1000.0 + (draw0 + np.arange(nd))[None, :, None] * 10.0 + np.arange(w)[None, None, :] + seed * 1e6).astype(np.float32)
        bad = (gi == self.OUT) | (gi >= self.total)
        out[bad] = np.nan
        if comp is not None:
            comp[:] = ((gi[None, :] + np.arange(nd)[:, None]) % self.K_FAKE).astype(np.int32)
            comp[:, bad] = -1
        return int(bad.sum())


@functools.lru_cache(maxsize=None)
def setup(Do, Dt, K, n=rd.N):
    """The case, and what a worker would hold for it (through a Regressor over the stand-in worker): the joint model, the marginal table in
    Float64 and the bound of its entries."""
    score = importlib.import_module(load_package().__name__ + ".host.score")
    c = rd.make_case(Do, Dt, K, n=n)
    with score.Predictor(rr.dummy_model(c["post"], K, c["D"]), capacity=40, worker_factory=StandIn) as parent:
        with parent.regressor(c["given"], c["targets"], worker_factory=StandIn) as reg:
            m, R = reg._joint_parameters()
            tabs = reg.tables(factor=True)
            mm, Rm, ld, dff, w = (np.asarray(a, np.float32) for a in reg.marginal._predictive_args()[1])
            W_set = reg.marginal._wk.W
    want, parts = pr.student_t_table(c["X"], mm, Rm, ld, dff, w)
    parts["want"] = want
    t = pr.error_bound(c["X"], mm, Rm, dff, parts).T
    return dict(c=c, m=m, R=R, tabs=tabs, df=dff.astype(np.float64), want=want, t=t, W_set=W_set)


def emulate(s, ref, seed, ndraws, mutate=None, side="covariance"):
    """What a kernel with the planted mistake would return: the other side of the reference, mutated, with its own components."""
    got = rd.draw(s["c"]["X"], s["m"], s["R"], s["df"], s["want"], np.arange(s["c"]["n"]), ndraws, seed, side=side, mutate=mutate)
    return got["x"].astype(np.float32), got["own"]


@pytest.mark.parametrize("Do,Dt,K", [(3, 2, 3), (33, 31, 3), (16, 17, 1), (1, 255, 3), (64, 64, 24)])
def test_two_sides_agree_and_mutations_are_rejected(Do, Dt, K):
    s = setup(Do, Dt, K)
    n, idx = s["c"]["n"], np.arange(s["c"]["n"])
    SEED = rd.case_seed(Do, Dt, K)
    a = rd.draw(s["c"]["X"], s["m"], s["R"], s["df"], s["want"], idx, 3, SEED, t=s["t"])
    b = rd.draw(s["c"]["X"], s["m"], s["R"], s["df"], s["want"], idx, 3, SEED, side="covariance")
    assert a["part"].all() and np.array_equal(a["own"], b["own"])
    scale = np.abs(a["x"]).max()
    assert np.abs(a["x"] - b["x"]).max() <= 1e-9 * scale
    if K > 1:
        assert len(np.unique(a["own"][:, :rd.TILE])) > 1, "the first tile holds one component: the clusters do not overlap"
    rel = rd.relative_table_error(s["t"], K)
    # the honest kernel (the other side, rounded to Float32) passes the GPU test's comparison; the seed excuses below 1 %
    got, comp = emulate(s, a, SEED, 3)
    ref = rd.draw(s["c"]["X"], s["m"], s["R"], s["df"], s["want"], idx, 3, SEED, comp=comp, t=s["t"])
    ratio, exc, wrong = rd.compare(got, comp, ref, rel)
    assert ratio <= 1.0 and exc <= rd.MAX_EXCUSED and wrong == 0, (ratio, exc, wrong)
    for mut in rd.MUTATIONS:
        if mut == "Li_not_transposed" and Dt == 1:
            continue
        got, comp = emulate(s, a, SEED, 3, mutate=mut)
        ratio, _, wrong = rd.compare(got, comp, rd.draw(s["c"]["X"], s["m"], s["R"], s["df"], s["want"], idx, 3, SEED, comp=comp, t=s["t"]), rel)
        assert ratio > 1.0 or wrong > 0, mut


@pytest.mark.parametrize("Do,Dt,K", rd.CASES)
def test_seeds_of_the_gpu_cases_excuse_below_one_percent(Do, Dt, K):
    from tools import impute_draw_ref as idr
    s = setup(Do, Dt, K)
    idx = np.arange(s["c"]["n"])
    p, rel = idr.probabilities(s["want"]), rd.relative_table_error(s["t"], K)
    exc = np.stack([idr.excused(p, rd.uniform(idx, j, rd.case_seed(Do, Dt, K)), rel) for j in range(3)])
    assert exc.mean() <= rd.MAX_EXCUSED, exc.mean()


@pytest.mark.parametrize("Do,Dt", rd.LAW_SHAPES)
def test_law_of_the_reference(Do, Dt):
    s = setup(Do, Dt, 1, n=rd.LAW_POINTS)
    n = s["c"]["n"]
    ref = rd.draw(s["c"]["X"], s["m"], s["R"], s["df"], s["want"], np.arange(n), rd.LAW_DRAWS, rd.LAW_SEED[(Do, Dt)])
    tb = ref["tables"]
    mu = tb["c"][0][None] + s["c"]["X"].astype(np.float64) @ tb["B"][0].T
    stat = rd.law_statistic(ref["x"], mu, tb["S"][0], s["df"][0], ref["q"][:, 0], Do)
    assert stat.size == 16384
    d, lim = rd.check_law(stat, Dt, s["df"][0] + Do)
    print(f"Do={Do} Dt={Dt}: KS distance {d:.5f} < {lim:.5f}")
    for mut in ("no_q", "chi_df"):
        bad = rd.draw(s["c"]["X"], s["m"], s["R"], s["df"], s["want"], np.arange(n), rd.LAW_DRAWS, rd.LAW_SEED[(Do, Dt)], mutate=mut)
        with pytest.raises(AssertionError):
            rd.check_law(rd.law_statistic(bad["x"], mu, tb["S"][0], s["df"][0], ref["q"][:, 0], Do), Dt, s["df"][0] + Do)


@pytest.mark.parametrize("Do,Dt,K", [(3, 2, 3), (33, 31, 3), (100, 156, 1)])
def test_factor_of_condition_py(cond, Do, Dt, K):
    s = setup(Do, Dt, K)
    B, c, V, h, df, W = s["tabs"]
    assert W.shape == (K, Dt, Dt) and np.array_equal(W, np.triu(W)) and np.array_equal(W, s["W_set"])
    assert len(cond.regression_tables(s["m"], s["R"], range(Do), range(Do, Do + Dt))) == 3
    for side in ("precision", "covariance"):
        tb = rd.tables(s["m"], s["R"], Do, side)
        assert np.abs(W - tb["W"]).max() <= 1e-8 * np.abs(W).max() and np.abs(B - tb["B"]).max() <= 1e-8 * max(1e-300, np.abs(B).max())
    WW = np.einsum("kij,klj->kil", W, W)
    assert np.allclose(np.einsum("kii->ki", WW), V, rtol=1e-10)
    # against regress_ref.dense_form: one point, one cluster at a time -- the conditional variance it reports is (df + q) / (df + D_o - 2) diag(W W')
    R3 = s["m"].shape[1]
    x = s["c"]["X"][:1].astype(np.float64)
    for k in range(K):
        p = np.zeros((1, K))
        p[0, k] = 1.0
        _, std = rr.dense_form(p, s["m"], s["R"].reshape(K, R3, R3), df, list(range(Do)), list(range(Do, Do + Dt)), x)
        q = rr.quad(x, s["m"][:, :Do], np.linalg.cholesky(rd.tables(s["m"], s["R"], Do)["Soo_inv"]).transpose(0, 2, 1))[0, k]
        assert np.allclose(std[0] ** 2, (df[k] + q) / (df[k] + Do - 2.0) * np.diag(WW[k]), rtol=1e-8)


def test_python_walk_and_argument_checks(score):
    c = rd.make_case(3, 2, StandIn.K_FAKE, n=93)
    data = np.ascontiguousarray(c["X"].T)
    with score.Predictor(rr.dummy_model(c["post"], c["K"], c["D"]), capacity=40, worker_factory=StandIn) as parent:
        reg = parent.regressor(c["given"], c["targets"], worker_factory=StandIn)
        reg.marginal._wk.total = 93
        for bad in (0, -1, 1.5, (1 << 26) + 1):
            with pytest.raises(ValueError, match="draws"):
                reg.sample(data, draws=bad)
        for bad in (-1, 1 << 64):
            with pytest.raises(ValueError, match="seed"):
                reg.sample(data, seed=bad)
        with pytest.raises(ValueError):
            reg.sample(data[:2])
        res = reg.sample(data, draws=4, seed=0, return_components=True)
        assert isinstance(res, score.RegressionDraws) and res.values.shape == (4, 2, 93) and res.values.dtype == np.float32
        assert res.components.shape == (4, 93) and res.components.dtype == np.int32 and res.labels.shape == (93,) and res.skipped == 1
        gi, j, d = np.arange(93)[None, None, :], np.arange(4)[:, None, None], np.arange(2)[None, :, None]
        want = (gi * 1000.0 + j * 10.0 + d).astype(np.float32)
        keep = np.arange(93) != StandIn.OUT
        assert np.array_equal(res.values[:, :, keep], want[:, :, keep]) and np.isnan(res.values[:, :, StandIn.OUT]).all()
        assert np.array_equal(res.components[:, keep], ((np.arange(93)[None, :] + np.arange(4)[:, None]) % 3)[:, keep]) and (res.components[:, StandIn.OUT] == -1).all()
        plain = reg.sample(data, draws=2)
        assert plain.components is None and np.array_equal(plain.values[:, :, keep], want[:2][:, :, keep]) and plain.skipped == 1
        mod = importlib.import_module(score.__name__.rsplit(".", 1)[0])
        assert mod.regress_sample is score.regress_sample and mod.RegressionDraws is score.RegressionDraws
        reg.close()
        with pytest.raises(RuntimeError, match="closed"):
            reg.sample(data)

    class NoDraws(FakeWorker):
        set_predictive_niw = set_option = lambda self, *a: None

        def set_regression(self, *a):
            pass
    with score.Predictor(rr.dummy_model(c["post"], c["K"], c["D"]), capacity=40, worker_factory=NoDraws) as parent:
        with parent.regressor(c["given"], c["targets"], worker_factory=NoDraws) as reg:
            with pytest.raises(RuntimeError, match="cannot draw"):
                reg.sample(data)


# ------------------------------------------------------------------------------------------------ the C boundary
def test_header_compiles_as_c_and_is_bound_exported_and_built(pkg):
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER])
    hdr = open(HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", body))) == FUNCS
    binding = importlib.import_module(pkg.__name__ + ".binding")
    assert sorted(n for n, _, _ in binding.ABI_REGRESS_DRAW) == FUNCS
    assert int(re.search(r"#define DPMM_REGRESS_MAX_DRAWS (\d+)", hdr).group(1)) == binding.REGRESS_MAX_DRAWS == 1 << 26
    csrc = os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "build/regress_draw.o" in re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "../../include/dpmm_hip_regress_draw.h" in re.search(r"^build/dpmm_api\.o:(.*)$", mk, flags=re.M).group(1).split()
    hip = open(os.path.join(csrc, "regress_draw.hip")).read()
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in hip and '#include "score_device.h"' in hip and not re.search(r"\batomic\w*\(", hip)
    dev = open(os.path.join(csrc, "dpmm_device.h")).read()
    assert "STREAM_REGRESS_COMP = 46, STREAM_REGRESS_NORMAL = 47, STREAM_REGRESS_CHI = 48" in dev
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for n in FUNCS:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                                   # additive: the version stays
