"""CPU-side checks of missing features (include/dpmm_hip_missing.h): the reference of tests/test_gpu_missing.py itself -- its two Float64
forms agree, the numpy restatement of the kernel is inside the derived bound, every planted mistake is outside it, the bound is not
vacuous -- then host/score.py's `missing=` keyword, `missing_counts` and `impute` over a stand-in worker defined here, and the C boundary
of the new header."""
import ctypes
import functools
import importlib
import os
import re
import subprocess
import types

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package
from tools import missing_ref as mr
from tools import predictive_ref as pr

HEADER = os.path.join(ROOT, "include", "dpmm_hip_missing.h")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


CORRELATED = ("correlated", 3)      # stands for mr.make_correlated_case() in the lists of cases below
ALL_CASES = mr.CASES + (CORRELATED,)


@functools.lru_cache(maxsize=None)
def case_ref(D, K):
    """(case with many gaps, its reference): computed once, shared, never modified."""
    c = mr.make_correlated_case() if (D, K) == CORRELATED else mr.make_case(D, K, dense=True)
    return c, mr.reference(c["X"], c["m"], c["R"], c["logdet"], c["df"], c["w"])


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("D,K", mr.CASES)
def test_the_two_float64_forms_agree(D, K):
    c = mr.make_case(D, K, dense=True)
    R64 = c["R"].astype(np.float64)
    logdet = -2 * np.log(np.abs(np.einsum("kii->ki", R64))).sum(1)                     # of the R in use, not its Float32 rounding
    ref = mr.reference(c["X"], c["m"], c["R"], logdet, c["df"], c["w"], exact_logdet=True)
    Sigma = np.linalg.inv(np.einsum("kji,kjl->kil", R64, R64))
    m64, df64, w64 = (c[k].astype(np.float64) for k in ("m", "df", "w"))
    X64 = c["X"].astype(np.float64)
    pts = np.flatnonzero(ref["check"])
    assert {0, c["n"] - 1, 50, c["mean_gap"]} <= set(pts.tolist()) and not ref["check"][c["naninf"]] and ref["listed"][c["naninf"]]
    pts = pts if D <= 64 else pts[:: max(1, len(pts) // 40)]                          # (a D x D solve per point and cluster)
    worst_t = worst_c = 0.0
    for i in pts:
        want, cm = mr.point_covariance(X64[i], ref["miss"][i], m64, Sigma, df64, w64)
        worst_t = max(worst_t, float((np.abs(want - ref["want"][:, i]) / (1 + np.abs(want))).max()))
        worst_c = max(worst_c, float((np.abs(cm - ref["cm"][int(i)]) / (1 + np.abs(cm))).max()))
    print(f"D={D} K={K}: {len(pts)} points, precision side against covariance side: table {worst_t:.2e}, conditional mean {worst_c:.2e} (relative)")
    assert worst_t < 1e-10 and worst_c < 1e-10
    # the classes: r = D and r = 17 are over the cap and stay NaN
    assert ref["over"][52] and np.isnan(ref["want"][:, 52]).all() and (D < 18 or ref["over"][51])
    assert int(ref["listed"].sum()) + int(ref["over"].sum()) == len(c["gaps"])


@pytest.mark.parametrize("D,K", ALL_CASES)
def test_the_restatement_is_inside_the_bound(D, K):
    c, ref = case_ref(D, K)
    table, cm = mr.emulate(c["X"], c["m"], c["R"], c["logdet"], c["df"], c["w"])
    a, b = mr.worst_ratios(table, cm, ref)
    print(f"D={D} K={K}: restatement, max error / bound: table {a:.3f}, conditional mean {b:.3f}")
    assert a <= 1.0 and b <= 1.0


@pytest.mark.parametrize("mutation", mr.MUTATIONS)
def test_every_planted_mistake_is_outside_the_bound(mutation):
    caught = []
    for D, K in ALL_CASES:
        c, ref = case_ref(D, K)
        a, b = mr.worst_ratios(*mr.emulate(c["X"], c["m"], c["R"], c["logdet"], c["df"], c["w"], mutation=mutation), ref)
        if a > 1.0 or b > 1.0:
            caught.append((D, K, round(min(a, 1e30), 1), round(min(b, 1e30), 1)))
    print(f"{mutation}: outside the bound in {len(caught)} of {len(ALL_CASES)} cases: {caught}")
    assert caught


@pytest.mark.parametrize("D,K", mr.CASES)
def test_the_bound_is_not_vacuous(D, K):
    """Over the marginalised bulk points, under the cluster each was drawn from, the bound is within test_loglik_table's tolerance for 95 %."""
    c, ref = case_ref(D, K)
    pts = np.flatnonzero(ref["check"] & c["bulk"])
    assert len(pts) >= 50
    own = c["lab"][pts]
    ok = ref["bound"][own, pts] <= pr.LOGLIK_ATOL + pr.LOGLIK_RTOL * np.abs(ref["want"][own, pts])
    print(f"D={D} K={K}: {len(pts)} marginalised bulk points, share inside the tolerance {ok.mean():.3f}")
    assert ok.mean() >= 0.95


def test_derived_tolerances_on_a_case_by_hand():
    """derived(): the probabilities sum to 1, the log-density is the log-sum-exp, an imputed value lies between the clusters' conditional means."""
    c, ref = case_ref(5, 3)
    d = mr.derived(ref)
    i = 50
    assert np.isclose(d["probs"][i].sum(), 1.0) and np.isclose(d["logdens"][i], np.log(np.exp(ref["want"][:, i]).sum()))
    lo, hi = ref["cm"][i].min(0), ref["cm"][i].max(0)
    assert np.all(d["fill"][i] >= lo - 1e-12) and np.all(d["fill"][i] <= hi + 1e-12) and np.all(d["fill_tol"][i] > 0)
    assert np.isnan(d["logdens"][52]) or np.isneginf(d["logdens"][52])


# ------------------------------------------------------------------------------------------------ the Python layer over a stand-in
class StandIn:
    """A worker that records what a Predictor asks of it.  Scores: a_k(i) = log w_k - |x_i - c_k|^2 over the features the point has when the
    option is on, NaN rows else; impute fills a gap with 100 + the sum of the point's other features; counts: rows with 1 .. D - 1 / D NaNs."""
    made = []

    def __init__(self, prior, D, n_local, first_index=0, device=0, seed=0):
        self.prior, self.D, self.n = prior, D, n_local
        self.options, self.uploads, self.closed, self.last = [], 0, False, (0, 0)
        StandIn.made.append(self)

    def close(self):
        self.closed = True

    def set_option(self, key, value):
        self.options.append((key, value))

    def upload_points(self, X):
        assert X.shape == (self.n, self.D) and X.dtype == np.float32
        self.X = np.array(X)
        self.uploads += 1

    def set_predictive_niw(self, m, R, logdet, df, weights):
        self.centres, self.logw, self.K = np.asarray(m, np.float64), np.log(np.asarray(weights, np.float64)), len(weights)

    def set_predictive_mult(self, logp, weights):
        self.set_predictive_niw(logp, None, None, None, weights)

    def set_projection(self, W, mu=None):
        self.D_in = W.shape[0]

    def upload_points_projected(self, X):
        raise AssertionError("projected upload with missing features")

    def _count(self):
        r = np.isnan(self.X).sum(1)
        self.last = (int(((r >= 1) & (r < self.D)).sum()), int((r == self.D).sum()))

    def score_points_into(self, outs, m=0):
        on = any(k == 33 and v for k, v in self.options)
        d = (self.X[:, None, :].astype(np.float64) - self.centres[None, :, :]) ** 2
        a = self.logw[None, :] - (np.nansum(d, -1) if on else d.sum(-1))
        self.last = (0, 0)
        if on:
            self._count()
        for name, arr in outs.items():
            arr[...] = dict(labels=np.argmax(np.where(np.isnan(a), np.inf, a), 1) + 1, logdens=np.log(np.exp(a).sum(1)))[name]

    def score_missing_counts(self):
        return self.last

    def impute_points_into(self, out):
        assert out.shape == (self.n, self.D) and out.dtype == np.float32
        fill = (100 + np.nansum(self.X, 1))[:, None]
        out[...] = np.where(np.isnan(self.X), fill, self.X)
        self._count()


def model(kind, D, K, seed=0, projection=None):
    rng = np.random.default_rng(seed)
    if kind == 0:
        A = rng.standard_normal((3 * K, D, D)) * 0.1 + np.eye(D)
        post = dict(kappa=1 + rng.random(3 * K), nu=D + 3 + rng.random(3 * K), m=rng.standard_normal((3 * K, D)), U=np.triu(A) + 2 * np.eye(D),
                    logdet_psi=np.zeros(3 * K))
    else:
        post = dict(alpha=(1 + rng.random((3 * K, D))).astype(np.float32))
    s = types.SimpleNamespace(K=K, prior=types.SimpleNamespace(kind=kind, dim=D), post=post, alpha=10.0, points_count=rng.integers(5, 50, K),
                              wk=types.SimpleNamespace(device=0))
    mdl = types.SimpleNamespace(sampler=s)
    if projection is not None:
        mdl.projection = projection
    return mdl


def gappy(D, n, seed=1):
    X = np.random.default_rng(seed).standard_normal((D, n)).astype(np.float32)
    for j, i in ((0, 3), (1, 4), (2, 4), (0, 17), (1, 33)):         # one gap, two gaps, then slabs 1 and 3 of capacity 10
        if i < n:
            X[j, i] = np.nan
    X[:, 25:26] = np.nan                                            # every feature: over the cap
    return X


def test_the_keyword_sets_the_option_once_and_counts_sum_over_slabs(score, pkg):
    binding = importlib.import_module(pkg.__name__ + ".binding")
    D, K, n, cap = 3, 4, 37, 10
    X = gappy(D, n)
    with score.Predictor(model(0, D, K), capacity=cap, worker_factory=StandIn, missing="marginalize") as p:
        wk = p._wk
        assert p.missing == "marginalize" and p.missing_counts == (0, 0)
        ld = p.score_samples(X)
        assert wk.uploads == 4 and p.missing_counts == (4, 1)                   # slabs hold (2, 0), (1, 0), (0, 1), (1, 0)
        lab = p.predict_labels(X)
        assert p.missing_counts == (4, 1) and lab.shape == (n,)
        assert np.isfinite(ld[[3, 4, 17, 33]]).all() and p.predict_labels(X[:, :10]).shape == (10,) and p.missing_counts == (2, 0)
        assert wk.options == [(binding.OPT_SCORE_MISSING, 1)] and binding.OPT_SCORE_MISSING == 33
    with score.Predictor(model(0, D, K), capacity=cap, worker_factory=StandIn) as p:       # the default: the worker is told nothing
        assert p.missing == "propagate" and np.isnan(p.score_samples(X)[[3, 4, 17, 25, 33]]).all()
        assert p._wk.options == [] and p.missing_counts == (0, 0)
    ld2 = score.score_samples(model(0, D, K), X, capacity=cap, worker_factory=StandIn, missing="marginalize")      # the one-shots pass it on
    assert np.array_equal(ld, ld2, equal_nan=True) and StandIn.made[-1].closed


def test_refusals(score):
    with pytest.raises(ValueError, match="missing"):
        score.Predictor(model(0, 3, 4), capacity=10, worker_factory=StandIn, missing="drop")
    with pytest.raises(ValueError, match="Multinomial"):
        score.Predictor(model(1, 3, 4), capacity=10, worker_factory=StandIn, missing="marginalize")
    with score.Predictor(model(1, 3, 4), capacity=10, worker_factory=StandIn) as p:
        with pytest.raises(ValueError, match="Multinomial"):
            p.impute(np.ones((3, 5), np.float32))
    # a model with a projection: D_in-row data has nothing to marginalise over; d-row data is served
    proj = types.SimpleNamespace(D_in=6, apply=lambda wk: wk.set_projection(np.zeros((6, 3))), arrays=lambda prefix: {})
    with score.Predictor(model(0, 3, 4, projection=proj), capacity=10, worker_factory=StandIn, missing="marginalize") as p:
        with pytest.raises(ValueError, match="projected coordinates"):
            p.score_samples(np.zeros((6, 5), np.float32))
        with pytest.raises(ValueError, match="projected coordinates"):
            p.impute(np.zeros((6, 5), np.float32))
        assert p.score_samples(gappy(3, 12)).shape == (12,) and p.missing_counts == (2, 0)
    with score.Predictor(model(0, 3, 4, projection=proj), capacity=10, worker_factory=StandIn) as p:
        with pytest.raises(ValueError, match="projected coordinates"):
            p.impute(np.zeros((6, 5), np.float32))
    p = score.Predictor(model(0, 3, 4), capacity=10, worker_factory=StandIn)
    p.close()
    with pytest.raises(RuntimeError, match="closed"):
        p.impute(np.zeros((3, 5), np.float32))


@pytest.mark.parametrize("n", [0, 9, 10, 37])
@pytest.mark.parametrize("mode", ["propagate", "marginalize"])
def test_impute_stitches_the_slabs_in_order(score, n, mode):
    D, K, cap = 3, 4, 10
    X = gappy(D, 37)[:, :n]
    with score.Predictor(model(0, D, K), capacity=cap, worker_factory=StandIn, missing=mode) as p:
        got = p.impute(X)
        assert p._wk.uploads == -(-n // cap)
        want_counts = (int(((np.isnan(X).sum(0) >= 1) & (np.isnan(X).sum(0) < D)).sum()), int((np.isnan(X).sum(0) == D).sum()))
        assert p.missing_counts == want_counts
    assert isinstance(got, np.ndarray) and got.shape == (D, n) and got.dtype == np.float32
    want = np.where(np.isnan(X), (100 + np.nansum(X, 0))[None, :], X).astype(np.float32)
    assert np.array_equal(got, want)
    host = importlib.import_module(score.__name__.rsplit(".", 1)[0])
    assert host.impute is score.impute
    assert np.array_equal(score.impute(model(0, D, K), X, capacity=7, worker_factory=StandIn), want)


def test_save_and_load_keep_working(score, tmp_path):
    p = score.Predictor(model(0, 3, 4, seed=5), capacity=7, worker_factory=StandIn, missing="marginalize")
    path = str(tmp_path / "model.npz")
    p.save(path)
    q = score.Predictor.load(path, capacity=5, worker_factory=StandIn, missing="marginalize")
    r = score.Predictor.load(path, capacity=5, worker_factory=StandIn)
    assert q.missing == "marginalize" and q._wk.options == [(33, 1)] and r.missing == "propagate" and r._wk.options == []
    X = gappy(3, 12)
    assert np.array_equal(p.score_samples(X), q.score_samples(X)) and q.missing_counts == (2, 0)
    with pytest.raises(ValueError, match="missing"):
        score.Predictor.load(path, worker_factory=StandIn, missing="zero")
    p.close(); q.close(); r.close()


# ------------------------------------------------------------------------------------------------ the C boundary
def test_header_compiles_as_c_and_is_bound_exported_and_built(pkg):
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER])
    hdr = open(HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", body)))
    assert declared == ["dpmm_impute_points", "dpmm_impute_points_device", "dpmm_score_missing_counts"]
    binding = importlib.import_module(pkg.__name__ + ".binding")
    assert sorted(n for n, _, _ in binding.ABI_MISSING) == declared
    assert not set(declared) & set(n for n, _, _ in binding.ABI + binding.ABI_TENSOR + binding.ABI_SCORE + binding.ABI_RANK + binding.ABI_CSC + binding.ABI_SAMPLE
                                   + binding.ABI_PROJECT)
    assert int(re.search(r"#define DPMM_OPT_SCORE_MISSING (\d+)", hdr).group(1)) == binding.OPT_SCORE_MISSING
    assert int(re.search(r"#define DPMM_SCORE_MAX_MISSING (\d+)", hdr).group(1)) == binding.SCORE_MAX_MISSING == mr.MAX_MISSING
    # the key is free: no other header gives 33 to an option
    for h in os.listdir(os.path.join(ROOT, "include")):
        src = open(os.path.join(ROOT, "include", h)).read()
        keys = re.findall(r"\b(DPMM_OPT_[A-Z0-9_]+)\s*=?\s+(\d+)\s*[,/\n]", src)
        assert [k for k, v in keys if int(v) == binding.OPT_SCORE_MISSING and k != "DPMM_OPT_SCORE_MISSING"] == [], h
    mk = open(os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "build/missing.o" in objs and re.search(r"^build/dpmm_api\.o:.*dpmm_hip_missing\.h", mk, flags=re.M)
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for n in declared:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                               # additive: the version stays
    for name in ("score_missing_counts", "impute_points_into"):
        assert callable(getattr(binding.Worker, name)), name
