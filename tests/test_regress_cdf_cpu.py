"""CPU-side checks of the conditional CDF and quantiles of the targets (include/dpmm_hip_regress_cdf.h): the Student-t quantiles of
host/condition.py against scipy, the reference of tests/test_gpu_regress_cdf.py itself -- the closed form at one cluster, the bimodal median,
the planted mistakes outside the bound, the PIT values of the law test's model --, the argument checks and the walk of the Python surface
over a stand-in worker, and the C boundary.  Float64, no GPU."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import stats

from __graft_entry__ import load_package
from fake_worker import FakeWorker
from tools import regress_cdf_ref as rc
from tools import regress_ref as rr
from test_integration_layout import _ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dpmm_hip_regress_cdf.h")
FUNCS = ["dpmm_regress_cdf_points", "dpmm_regress_cdf_points_device", "dpmm_regress_quantile_points", "dpmm_regress_quantile_points_device",
         "dpmm_set_regression_levels"]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


@pytest.fixture(scope="module")
def cond(pkg):
    return importlib.import_module(pkg.__name__ + ".host.condition")


def test_student_t_ppf(cond):
    nu = np.array([1.0, 2.5, 30.0, 1e4, 1e7])
    lv = np.array([1e-6, 1e-4, 0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 1 - 1e-4, 1 - 1e-6])
    z = cond.student_t_ppf(lv, nu)
    ref = stats.t.ppf(lv[None, :], nu[:, None])
    assert z.shape == (5, 11) and z.dtype == np.float64
    assert np.all(np.abs(z - ref) <= 1e-10 * np.abs(ref) + 1e-14)
    assert np.all(z[:, 5] == 0.0)                                        # exactly 0 at 1 / 2
    assert np.array_equal(z[:, 4], -z[:, 6])                             # antisymmetric (0.25 and 0.75 are exact complements)
    assert np.all(np.abs(z + z[:, ::-1]) <= 1e-9 * np.abs(z))            # (1 - 1e-6 is not exactly the complement of 1e-6)
    assert np.all(np.diff(z, axis=1) > 0)
    # in probability: the library's own tail at the quantile gives the level back
    back = 0.5 * cond.student_t_tail(z[:, :5], nu[:, None])
    assert np.all(np.abs(back - lv[None, :5]) <= 1e-9 * lv[None, :5])      # (far below u = 2^-24, the rounding of a quantile)
    for bad in ([0.0], [1.0], [-0.1], [np.nan]):
        with pytest.raises(ValueError):
            cond.student_t_ppf(bad, nu)


class StandIn(FakeWorker):
    """A worker that records what it is handed and returns functions of (global index, level / target): what the walk has to put in place."""
    K_FAKE = 3
    OUT = 41

    def set_predictive_niw(self, *a):
        pass

    def set_option(self, *a):
        pass

    def set_regression(self, B, c, V, h):
        self.reg = (B, c, V, h)
        self.levels = None

    def regress_cdf_points_into(self, y, cdf, sf=None, labels=None):
        assert y.dtype == np.float32 and y.flags.c_contiguous and y.shape == cdf.shape
        self.calls = getattr(self, "calls", 0) + 1
        cdf[:] = y + 0.25
        sf[:] = 0.75 - y
        labels[:] = 1 + (np.arange(len(labels)) % self.K_FAKE)
        bad = y[:, 0] == self.OUT
        cdf[bad] = np.nan
        return int(bad.sum())

    def set_regression_levels(self, levels, z):
        self.levels, self.z = np.array(levels), np.array(z)
        self.handed = getattr(self, "handed", 0) + 1

    def regress_quantile_points_into(self, out, labels=None):
        n, L, w = out.shape
        assert L == len(self.levels)
        out[:] = (self.levels[None, :, None] * 100.0 + np.arange(w)[None, None, :]).astype(np.float32)
        labels[:] = 2
        return 0


def stand_in_regressor(score, c, factory=StandIn):
    parent = score.Predictor(rr.dummy_model(c["post"], c["K"], c["D"]), capacity=40, worker_factory=factory)
    return parent, parent.regressor(c["given"], c["targets"], worker_factory=factory)


def tables_of(score, c):
    parent, reg = stand_in_regressor(score, c)
    with parent, reg:
        B, cc, V, h, df = reg.tables()
        m = np.asarray(reg.marginal._predictive_args()[1][0], np.float32).astype(np.float64)
        R = np.asarray(reg.marginal._predictive_args()[1][1], np.float32).astype(np.float64).reshape(c["K"], c["Do"], c["Do"])
    return dict(B=B, c=cc, V=V, df=df, q=rr.quad(c["X"].astype(np.float64), m, R), x=c["X"].astype(np.float64))


def test_reference_at_one_cluster_is_the_closed_form(score):
    c = rc.make_case(5, 31, 1, 33)
    t = tables_of(score, c)
    p = np.ones((33, 1))
    q = rc.quantile(p, t["B"], t["c"], t["V"], t["df"], t["q"], t["x"], rc.LEVELS)
    mu, sig, nu = rc.components(t["B"], t["c"], t["V"], t["df"], t["q"], t["x"], 5)
    for j, lv in enumerate(rc.LEVELS):
        want = mu[:, 0] + sig[:, 0] * stats.t.ppf(lv, nu[0])
        assert np.all(np.abs(q[j] - want) <= 1e-9 * (np.abs(want) + sig[:, 0]))
        r = rc.cdf(p, t["B"], t["c"], t["V"], t["df"], t["q"], t["x"], q[j])
        assert np.all(np.abs(r["cdf"] - lv) <= 1e-12) and np.all(np.abs(r["cdf"] + r["sf"] - 1) <= 1e-15)


def test_reference_bimodal_median_lies_in_the_gap():
    """Two equal clusters whose conditional laws sit 40 apart: the median is between the modes, where the density is next to nothing,
    and the CDF there is still 1 / 2 -- the quantile is well conditioned in probability, not in y."""
    B, c, V, df = np.zeros((2, 1, 1)), np.array([[-20.0], [20.0]]), np.ones((2, 1)), np.array([30.0, 30.0])
    p, q, x = np.array([[0.5, 0.5]]), np.zeros((1, 2)), np.zeros((1, 1))
    med = rc.quantile(p, B, c, V, df, q, x, (0.5,))[0]
    assert abs(med[0, 0]) < 15.0
    r = rc.cdf(p, B, c, V, df, q, x, med)
    assert abs(r["cdf"][0, 0] - 0.5) <= 1e-12 and r["pdf"][0, 0] < 1e-12


@pytest.mark.parametrize("Do,Dt,K", [(1, 1, 3), (5, 31, 3), (33, 130, 3)])
def test_planted_mistakes_are_outside_the_bound(score, Do, Dt, K):
    c = rc.make_case(Do, Dt, K, 33)
    t = tables_of(score, c)
    l = np.log(rr.weights(10 + 5 * np.arange(K)))[None] - 0.5 * (t["df"] + Do)[None] * np.log1p(t["q"] / t["df"][None])      # (the shape of the table entries)
    p = np.exp(l - l.max(1, keepdims=True))
    p = (p / p.sum(1, keepdims=True)).astype(np.float32).astype(np.float64)
    assert Do > 5 or ((p > 1e-3).sum(1) > 1).any()
    ok = rc.cdf(p, t["B"], t["c"], t["V"], t["df"], t["q"], t["x"], c["Y"])
    assert np.all(np.abs(ok["cdf"] + ok["sf"] - p.sum(1, keepdims=True)) <= 1e-14)
    for mut in rc.MUTATIONS:
        bad = rc.cdf(p, t["B"], t["c"], t["V"], t["df"], t["q"], t["x"], c["Y"], mutation=mut)
        assert np.any(np.abs(bad["cdf"] - ok["cdf"]) > ok["b_cdf"]) and np.any(np.abs(bad["sf"] - ok["sf"]) > ok["b_sf"]), mut


def test_reference_pit_values_of_the_law_sample_pass_with_room(score):
    """The model AND the sample of the GPU law test (D = 6, K = 4, overlapping; `Predictor.sample(20000, seed)`): tools/sample_ref restates
    the sampler from the same random words -- the cluster sizes are the host's draw, the points those of the GPU up to its Float32
    arithmetic.  Their PIT values from the reference with exact probabilities lie below the Kolmogorov criterion with room, so that on the
    GPU only the kernel can fail it."""
    from tools import sample_ref as R
    L = rc.LAW
    post = rc.law_posterior()
    K, D, n = L["K"], L["D"], L["n"]
    with score.Predictor(rr.dummy_model(post, K, D), capacity=40, worker_factory=StandIn) as p:
        _, m, A, dfs = p.sampler_tables()
        lab = R.labels_of(p.cluster_sizes(n, L["seed"]))
        w = np.asarray(p.weights, np.float64)
    X = R.niw_points(m, A, dfs, lab, np.arange(n), L["seed"]).astype(np.float32).astype(np.float64)
    df = post["nu"] - D + 1
    assert np.allclose(dfs, df)
    S = [((post["kappa"][k] + 1) / (post["kappa"][k] * df[k])) * (post["U"][k] @ post["U"][k].T) for k in range(K)]
    O, M = L["given"], L["targets"]
    p = np.exp(rr.marginal_logdens(post, w / w.sum(), O, X[:, O]))
    p /= p.sum(1, keepdims=True)
    u = np.zeros((n, len(M)))
    for k in range(K):
        Soo, Smo, Smm = S[k][np.ix_(O, O)], S[k][np.ix_(M, O)], S[k][np.ix_(M, M)]
        G = Smo @ np.linalg.inv(Soo)
        z = X[:, O] - post["m"][k, O]
        q = np.einsum("ne,ef,nf->n", z, np.linalg.inv(Soo), z)
        mu = post["m"][k, M] + z @ G.T
        sig = np.sqrt(((df[k] + q) / (df[k] + len(O)))[:, None] * np.diag(Smm - G @ Smo.T)[None])
        u += p[:, k:k + 1] * stats.t.cdf((X[:, M] - mu) / sig, df[k] + len(O))
    assert ((p > 1e-3).sum(1) > 1).mean() > 0.5
    for d in range(len(M)):
        dist = rc.kolmogorov(u[:, d])
        print(f"target {d}: Kolmogorov distance {dist:.5f} against {L['limit']:.5f}")
        assert dist < 0.6 * L["limit"]                                   # (seeds 1 to 8 give 0.0058 to 0.0121 at worst; this one is the roomiest)


def test_python_walk_and_argument_checks(score):
    c = rc.make_case(3, 2, StandIn.K_FAKE, 93)
    data = np.ascontiguousarray(c["X"].T)
    y = np.arange(2 * 93, dtype=np.int64).reshape(93, 2).T.copy() % 50          # (an integer dtype: converted slab by slab)
    y[0, 41] = StandIn.OUT
    parent, reg = stand_in_regressor(score, c)
    with parent:
        res = reg.cdf(data, y)
        assert isinstance(res, score.ConditionalCDF) and res.cdf.shape == (2, 93) and res.cdf.dtype == np.float32 and res.skipped == 1
        keep = np.arange(93) != 41
        assert np.array_equal(res.cdf[:, keep], (y + 0.25).astype(np.float32)[:, keep]) and np.isnan(res.cdf[:, 41]).all()
        assert np.array_equal(res.sf, (0.75 - y).astype(np.float32)) and np.array_equal(res.labels, 1 + np.arange(93) % 40 % 3)
        assert reg.marginal._wk.calls == 3                                   # slabs of 40 points
        for bad in (np.zeros((2, 92)), np.zeros((3, 93)), np.zeros(93), np.zeros((2, 93), dtype=complex)):
            with pytest.raises((ValueError, TypeError)):
                reg.cdf(data, bad)
        for bad in ([0.0, 0.5], [0.5, 1.0], [-0.1], [1.5], [float("nan")]):
            with pytest.raises(ValueError, match="inside"):
                reg.quantile(data, bad)
        for bad in ([], list(np.linspace(0.01, 0.99, 17)), [[0.1, 0.2]]):
            with pytest.raises(ValueError, match="levels"):
                reg.quantile(data, bad)
        for bad in (0.0, 1.0, 1.5):
            with pytest.raises(ValueError):
                reg.interval(data, bad)
        qs = reg.quantile(data, (0.95, 0.05, 0.5))
        wk = reg.marginal._wk
        assert isinstance(qs, score.RegressionQuantiles) and qs.values.shape == (3, 2, 93) and qs.levels == (0.95, 0.05, 0.5) and qs.skipped == 0
        assert np.array_equal(wk.levels, [0.05, 0.5, 0.95]) and wk.z.shape == (3, 3) and np.all(wk.z[:, 1] == 0.0)
        df = reg.tables()[4]
        assert np.allclose(wk.z, stats.t.ppf(np.array([0.05, 0.5, 0.95])[None, :], (df + 3)[:, None]), rtol=1e-10, atol=1e-15)      # (scipy gives 7e-17 at 1 / 2)
        assert np.array_equal(qs.values[:, 1, 7], np.float32([96.0, 6.0, 51.0]))                  # in the order asked for
        lower, upper = reg.interval(data, 0.9)
        assert lower.shape == (2, 93) and np.allclose(lower[0], 5.0) and np.allclose(upper[0], 95.0)
        assert len(score.Regressor.quantile.__defaults__[0]) == 3
        reg.quantile(data, (0.05, 0.95))
        handed = wk.handed
        reg.quantile(data, (0.95, 0.05))                                     # the same levels again: not handed over twice
        assert wk.handed == handed
        reg._tables_for = None                                               # a refresh (as after marginal.absorb) takes the levels with it
        reg.quantile(data, (0.05, 0.95))
        assert wk.handed == handed + 1 and np.array_equal(wk.levels, [0.05, 0.95])
        mod = importlib.import_module(score.__name__.rsplit(".", 1)[0])
        assert mod.regress_cdf is score.regress_cdf and mod.regress_quantile is score.regress_quantile
        assert mod.ConditionalCDF is score.ConditionalCDF and mod.RegressionQuantiles is score.RegressionQuantiles
        reg.close()
        for call in (lambda: reg.cdf(data, y), lambda: reg.quantile(data), lambda: reg.interval(data)):
            with pytest.raises(RuntimeError, match="closed"):
                call()

    class Older(FakeWorker):
        set_predictive_niw = set_option = set_regression = lambda self, *a: None
    parent, reg = stand_in_regressor(score, c, Older)
    with parent, reg:
        with pytest.raises(RuntimeError, match="cannot give"):
            reg.cdf(data, y)
        with pytest.raises(RuntimeError, match="cannot give"):
            reg.quantile(data)


def test_y_as_a_tensor(score):
    """Host data takes y as a CPU tensor of any real dtype as it takes a numpy array; a tensor that lives elsewhere is refused."""
    torch = pytest.importorskip("torch")
    c = rc.make_case(3, 2, StandIn.K_FAKE, 93)
    data = np.ascontiguousarray(c["X"].T)
    y = (np.arange(2 * 93, dtype=np.int64).reshape(93, 2).T % 40).copy()
    parent, reg = stand_in_regressor(score, c)
    with parent, reg:
        want = reg.cdf(data, y)
        for t in (torch.as_tensor(y), torch.as_tensor(y).double(), torch.as_tensor(y).to(torch.bfloat16), torch.as_tensor(y.T.copy()).T):
            got = reg.cdf(data, t)
            assert isinstance(got.cdf, np.ndarray) and np.array_equal(got.cdf, want.cdf) and np.array_equal(got.sf, want.sf)
        with pytest.raises(ValueError, match="lives"):
            reg.cdf(data, torch.zeros((2, 93), device="meta"))
        with pytest.raises(ValueError):
            reg.cdf(data, torch.zeros((2, 92)))


# ------------------------------------------------------------------------------------------------ the C boundary
def test_header_compiles_as_c_and_is_bound_exported_built_and_matches_julia(pkg):
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER])
    hdr = open(HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", body))) == FUNCS
    binding = importlib.import_module(pkg.__name__ + ".binding")
    assert sorted(n for n, _, _ in binding.ABI_REGRESS_CDF) == FUNCS
    assert int(re.search(r"#define DPMM_REGRESS_MAX_LEVELS (\d+)", hdr).group(1)) == binding.REGRESS_MAX_LEVELS == 16
    protos = {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(dpmm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", body, flags=re.S)}
    for n, _, args in binding.ABI_REGRESS_CDF:
        assert len(args) == protos[n], n
    for f in ("regress_cdf_points_into", "set_regression_levels", "regress_quantile_points_into"):
        assert hasattr(binding.Worker, f)
    jl = open(os.path.join(ROOT, "julia", "gpu_regress_cdf.jl")).read()
    calls = _ccalls(jl)
    assert sorted(s for s, _, _ in calls) == FUNCS
    for sym, ntypes, nvals in calls:
        assert ntypes == protos[sym] and nvals == protos[sym], (sym, ntypes, nvals, protos[sym])
    csrc = os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "build/regress_cdf.o" in re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "../../include/dpmm_hip_regress_cdf.h" in re.search(r"^build/dpmm_api\.o:(.*)$", mk, flags=re.M).group(1).split()
    hip = open(os.path.join(csrc, "regress_cdf.hip")).read()
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in hip and '#include "score_device.h"' in hip and "typ_tail(" in hip and not re.search(r"\batomic\w*\(", hip)
    assert not re.search(r"\bwhile\s*\(", hip)                             # every loop has a trip count
    assert "dpmm_hip_regress_cdf.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for n in FUNCS:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                                   # additive: the version stays
