"""CPU-side checks of the imputation draws (include/dpmm_hip_impute.h): the reference of tests/test_gpu_impute_draws.py itself -- its two
Float64 routes agree, its chi^2 is sample_ref's, the law checks accept it and reject every planted mistake at the sizes the GPU test uses,
the seeds of the GPU test excuse almost no component -- then host/score.py's `impute(draws=...)` over a stand-in worker defined here, and
the C boundary of the new header."""
import ctypes
import functools
import importlib
import json
import os
import re
import subprocess
import types

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package
from tools import impute_draw_ref as ir
from tools import missing_ref as mr
from tools import sample_ref as sr

HEADER = os.path.join(ROOT, "include", "dpmm_hip_impute.h")
VALUE_SEED, VALUE_DRAWS = 11, 3             # tests/test_gpu_impute_draws.py: test_values_against_float64
LAW_SEED = 5                                # ... and test_the_law


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


CORRELATED = ("correlated", 3)
VALUE_CASES = tuple(c for c in mr.CASES if c[1] == 3) + (CORRELATED,)


@functools.lru_cache(maxsize=None)
def case_ref(D, K):
    c = mr.make_correlated_case() if (D, K) == CORRELATED else mr.make_case(D, K)
    return c, mr.reference(c["X"], c["m"], c["R"], c["logdet"], c["df"], c["w"])


# ------------------------------------------------------------------------------------------------ the reference itself
def test_the_chi2_restatement_is_sample_refs():
    idx = np.arange(500, dtype=np.uint64) + (1 << 33)
    for df in (0.7, 3.0, 61.0):
        assert np.array_equal(ir.chi2(df, idx, 9, stream=sr.STREAM_CHI, block0=0), sr.chi2(df, idx, 9))
    assert not np.array_equal(ir.chi2(61.0, idx, 9, block0=64), ir.chi2(61.0, idx, 9, block0=0))


@pytest.mark.parametrize("D,K", VALUE_CASES)
def test_the_two_float64_routes_agree(D, K):
    """Precision side (R[:, M], its Gram matrix, the residual) against covariance side (the explicit Sigma, the Schur complement, the
    textbook conditional mean), from the same random words and components.  Tolerance: the covariance side inverts R'R, solves with
    Sigma_OO and inverts the Schur complement -- each loses cond(Sigma) 2^-53 relative to the largest entry; 1000 cond(Sigma) 2^-52
    (1 + |x|) leaves the three steps and the growth with D a factor of some hundreds.  cond(Sigma) is computed from the case: below 10 for
    missing_ref.make_case, 4e4 for the correlated case."""
    c, ref = case_ref(D, K)
    pts = np.flatnonzero(ref["check"])
    pts = pts if c["D"] <= 64 else pts[:: max(1, len(pts) // 12)]
    idx = np.arange(c["n"], dtype=np.uint64) + 1000
    a = ir.draw(c, ref, idx, 2, VALUE_SEED, points=pts)
    b = ir.draw(c, ref, idx, 2, VALUE_SEED, points=pts, side="covariance", comp=a["comp"])
    R64 = c["R"].astype(np.float64).reshape(c["K"], c["D"], c["D"])
    cond = max(np.linalg.cond(R64[k]) ** 2 for k in range(c["K"]))
    tol = 1000 * cond * 2.0 ** -52
    worst = max(float((np.abs(a["x"][int(i)] - b["x"][int(i)]) / (1 + np.abs(a["x"][int(i)]))).max()) for i in pts)
    print(f"D={D} K={K}: {len(pts)} points x 2 draws, cond(Sigma) {cond:.3g}, precision side against covariance side {worst:.2e} (tolerance {tol:.2e})")
    assert np.array_equal(a["comp"], b["comp"]) and worst < tol


def test_the_component_rule_by_hand():
    p = np.array([[0.25, 0.0, 0.5, 0.25], [0.0, 0.0, 0.0, 0.0], [0.5, 0.5, 0.0, 0.0], [0.5, 0.25, 0.0, 0.0]])
    u = np.array([0.25, 0.3, 0.999, 0.9])
    k, _ = ir.pick(p, u)
    # 0.25 is not < 0.25: cluster 2 (cluster 1 has probability 0 and is skipped); all zero: cluster 0; 0.999 < 1: cluster 1; rounding left
    # no cluster: the last one of positive probability
    assert k.tolist() == [2, 0, 1, 1]
    assert ir.probabilities(np.array([[np.nan, 0.0], [np.nan, np.nan], [np.nan, 0.0]])).tolist() == [[0, 0, 0], [0.5, 0, 0.5]]


@pytest.mark.parametrize("D,K", VALUE_CASES)
def test_the_seed_of_the_gpu_test_excuses_almost_no_component(D, K):
    """At most 1 % of the (marginalised point, draw) pairs may lie within the table's Float32 bound of a cumulative edge."""
    c, ref = case_ref(D, K)
    der = mr.derived(ref)
    lst = np.flatnonzero(ref["check"])
    with np.errstate(all="ignore"):
        rel = (np.expm1(2 * ref["bound"].max(0)) + mr.EPS * (c["K"] + 16))[lst]
    p = ir.probabilities(ref["want"])[lst]
    assert np.allclose(p, der["probs"][lst])
    idx = np.arange(c["n"], dtype=np.uint64)
    ex = np.stack([ir.excused(p, ir.uniform(idx, j, VALUE_SEED)[lst], rel) for j in range(VALUE_DRAWS)])
    print(f"D={D} K={K}: {ex.sum()} of {ex.size} pairs excused, largest rel {rel.max():.2e}")
    assert ex.mean() <= 0.01


@functools.lru_cache(maxsize=None)
def law_ref(D, r, df):
    c = ir.law_case(D, r, df)
    return c, mr.reference(c["X"], c["m"], c["R"], c["logdet"], c["df"], c["w"]), {}


def law_verdict(D, r, df, mutate):
    """None if the law checks accept the (mutated) reference's draws at the GPU test's sizes, else the message of the check that failed."""
    c, ref, cache = law_ref(D, r, df)
    idx = np.arange(c["n"], dtype=np.uint64)
    good = ir.draw(c, ref, idx, ir.LAW_DRAWS, LAW_SEED, cache=cache) if mutate else None
    got = ir.draw(c, ref, idx, ir.LAW_DRAWS, LAW_SEED, mutate=mutate, cache=cache)
    truth = got if good is None else ir.draw(c, ref, idx, ir.LAW_DRAWS, LAW_SEED, comp=got["comp"], cache=cache)      # L, t, q_o of the clusters drawn
    df64 = c["df"].astype(np.float64)
    u = np.stack([ir.standardise(got["x"][i], truth["parts"][i], got["comp"][:, i], df64, D) for i in range(c["n"])])
    try:
        ir.check_law(u, got["comp"].T, df64 + D - r)
        ir.check_frequencies(got["comp"].T, (good or got)["p"])
    except AssertionError as e:
        return str(e)
    return None


@pytest.mark.parametrize("D,r,df", ir.LAW_CASES)
def test_the_law_checks_accept_the_reference(D, r, df):
    c, ref, _ = law_ref(D, r, df)
    assert ref["listed"].all() and (ref["r"] == r).all() and c["n"] * ir.LAW_DRAWS == 20000
    p = ir.probabilities(ref["want"])
    print(f"D={D} r={r}: mean probabilities {np.round(p.mean(0), 3).tolist()}")
    assert p.mean(0)[0] > 0.6 and p.mean(0)[1:].min() > 0.02          # one dominant cluster, the others really drawn
    assert law_verdict(D, r, df, None) is None


@pytest.mark.parametrize("mutate", ir.MUTATIONS)
def test_the_law_checks_reject_every_planted_mistake(mutate):
    verdicts = {(D, r): law_verdict(D, r, df, mutate) for D, r, df in ir.LAW_CASES}
    for k, v in verdicts.items():
        print(f"{mutate} at (D, r) = {k}: {v or 'accepted'}")
    assert any(verdicts.values())
    if mutate in ("no_qo", "chi_df"):                                  # the scale: the cases with D_o >= df must see it
        assert verdicts[(64, 4)] and verdicts[(130, 3)]


# ------------------------------------------------------------------------------------------------ the Python layer over a stand-in
LOG = []


class StandIn:
    """A worker that records what a Predictor asks of it, in the notation of tests/golden/points_calls.json.  A draw fills a gap with
    1000 seed + 100 (global index) + 10 (draw index) + feature, comp with the global index % 3."""

    def __init__(self, prior, D, n_local, first_index=0, device=0, seed=0):
        self.prior, self.D, self.n = prior, D, n_local
        LOG.append(["__init__", prior, D, n_local, dict(first_index=first_index, device=device, seed=seed)])

    def close(self):
        LOG.append(["close"])

    def set_predictive_niw(self, m, R, logdet, df, weights):
        LOG.append(["set_predictive_niw"] + [f"{np.asarray(a).dtype}{list(np.shape(a))}" for a in (m, R, logdet, df, weights)])

    def set_predictive_mult(self, logp, weights):
        pass

    def set_projection(self, W, mu=None):
        pass

    def upload_points(self, X):
        assert X.shape == (self.n, self.D) and X.dtype == np.float32
        self.X = np.array(X)
        LOG.append(["upload_points", f"{X.dtype}{list(X.shape)}"])

    def score_missing_counts(self):
        LOG.append(["score_missing_counts"])
        r = np.isnan(self.X).sum(1)
        return int(((r >= 1) & (r < self.D)).sum()), int((r == self.D).sum())

    def impute_points_into(self, out):
        LOG.append(["impute_points_into", f"{out.dtype}{list(out.shape)}"])
        out[...] = np.where(np.isnan(self.X), 0, self.X)

    def impute_draws_into(self, out, seed, i0, draw0=0, comp=None):
        LOG.append(["impute_draws_into", f"{out.dtype}{list(out.shape)}", seed, i0, draw0, None if comp is None else f"{comp.dtype}{list(comp.shape)}"])
        assert out.flags.c_contiguous and out.shape[0] == self.n and out.shape[2] == self.D
        i, j, f = np.meshgrid(np.arange(self.n), np.arange(out.shape[1]), np.arange(self.D), indexing="ij")
        r = np.isnan(self.X).sum(1)
        drawn = ((r >= 1) & (r < self.D))
        fill = (1000 * seed + 100 * (i0 + i) + 10 * (draw0 + j) + f).astype(np.float32)
        out[...] = np.where(np.isnan(self.X)[:, None, :] & drawn[:, None, None], fill, self.X[:, None, :])
        if comp is not None:
            comp[...] = np.where(drawn, (i0 + np.arange(self.n)) % 3, -1)[None, :]


def model(kind=0, D=3, K=2):
    rng = np.random.default_rng(7)
    if kind == 0:
        A = rng.standard_normal((3 * K, D, D)) * 0.1 + np.eye(D)
        post = dict(kappa=1 + rng.random(3 * K), nu=D + 3 + rng.random(3 * K), m=rng.standard_normal((3 * K, D)), U=np.triu(A) + 2 * np.eye(D),
                    logdet_psi=np.zeros(3 * K))
    else:
        post = dict(alpha=(1 + rng.random((3 * K, D))).astype(np.float32))
    s = types.SimpleNamespace(K=K, prior=types.SimpleNamespace(kind=kind, dim=D), post=post, alpha=10.0, points_count=np.array([5, 7]),
                              wk=types.SimpleNamespace(device=0))
    return types.SimpleNamespace(sampler=s)


def gappy(D, n):
    X = np.random.default_rng(1).integers(0, 4, (D, n)).astype(np.float32)
    for j, i in ((0, 1), (1, 2), (2, 2), (0, 5), (1, 8)):
        if i < n:
            X[j, i] = np.nan
    if n > 6:
        X[:, 6] = np.nan
    return X


def logged(score, data, **kw):
    del LOG[:]
    with score.Predictor(model(), capacity=4, worker_factory=StandIn) as p:
        out = p.impute(data, **kw)
        LOG.append(["missing_counts", list(p.missing_counts)])
    return out, json.loads(json.dumps(LOG))


def test_without_draws_the_worker_sees_the_calls_of_the_golden_file(score):
    with open(os.path.join(ROOT, "tests", "golden", "points_calls.json")) as f:
        golden = json.load(f)
    rows = golden["cases"]["Predictor.impute numpy"]["niw plain"]
    for n, i in zip((0, 1, 4, 5, 9), rows):
        out, log = logged(score, np.random.default_rng(n).integers(0, 4, (3, n)).astype(np.float64))
        want = [e for e in golden["logs"][i] if e[0] != "returns"]
        assert log == want, n
        assert out.shape == (3, n) and out.dtype == np.float32


@pytest.mark.parametrize("n", [0, 3, 4, 9])
def test_draws_walk_the_slabs_with_global_indices(score, n):
    D, m = 3, 2
    X = gappy(D, n)
    out, log = logged(score, X, draws=m, seed=6)
    (res, comp), log2 = logged(score, X, draws=m, seed=6, return_components=True)
    assert isinstance(out, np.ndarray) and out.shape == (m, D, n) and out.dtype == np.float32 and np.array_equal(out, res, equal_nan=True)
    assert comp.shape == (m, n) and comp.dtype == np.int32
    calls = [e for e in log if e[0] == "impute_draws_into"]
    assert calls == [["impute_draws_into", f"float32[4, {m}, {D}]", 6, lo, 0, None] for lo in range(0, n, 4)]
    assert [e for e in log2 if e[0] == "impute_draws_into"] == [c[:5] + [f"int32[{m}, 4]"] for c in calls]
    assert [e[0] for e in log if e[0] in ("upload_points", "impute_draws_into", "score_missing_counts")] == ["upload_points", "impute_draws_into", "score_missing_counts"] * len(calls)
    assert not [e for e in log if e[0] == "impute_points_into"]
    r = np.isnan(X).sum(0)
    drawn = (r >= 1) & (r < D)
    assert log[-2:] == [["missing_counts", [int(drawn.sum()), int((r == D).sum())]], ["close"]]
    for j in range(m):
        assert n == 0 or out[j].T.strides[1] == 4                            # the .T view of point-major memory
        for i in range(n):
            for f in range(D):
                want = 6000 + 100 * i + 10 * j + f if np.isnan(X[f, i]) and drawn[i] else X[f, i]
                assert out[j, f, i] == want or (np.isnan(want) and np.isnan(out[j, f, i]))
        assert comp[j].tolist() == [i % 3 if drawn[i] else -1 for i in range(n)]
    one = score.impute(model(), X, draws=m, seed=6, capacity=3, worker_factory=StandIn)        # the one-shot passes it on; capacity decides nothing
    assert np.array_equal(one, out, equal_nan=True)


def test_refusals(score):
    X = gappy(3, 5)
    with score.Predictor(model(), capacity=4, worker_factory=StandIn) as p:
        for bad in (0, -1, 1.5):
            with pytest.raises(ValueError, match="draws"):
                p.impute(X, draws=bad)
        with pytest.raises(ValueError, match="seed"):
            p.impute(X, draws=1, seed=-1)
        with pytest.raises(ValueError, match="return_components"):
            p.impute(X, return_components=True)
    with score.Predictor(model(kind=1), capacity=4, worker_factory=StandIn) as p:
        with pytest.raises(ValueError, match="Multinomial"):
            p.impute(np.ones((3, 5), np.float32), draws=2)
    proj = types.SimpleNamespace(D_in=6, apply=lambda wk: wk.set_projection(np.zeros((6, 3))), arrays=lambda prefix: {})
    mdl = model()
    mdl.projection = proj
    with score.Predictor(mdl, capacity=4, worker_factory=StandIn) as p:
        with pytest.raises(ValueError, match="projected coordinates"):
            p.impute(np.zeros((6, 5), np.float32), draws=2)
    p = score.Predictor(model(), capacity=4, worker_factory=StandIn)
    p.close()
    with pytest.raises(RuntimeError, match="closed"):
        p.impute(X, draws=2)


# ------------------------------------------------------------------------------------------------ the C boundary
def test_header_compiles_as_c_and_is_bound_exported_and_built(pkg):
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER])
    hdr = open(HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", body)))
    assert declared == ["dpmm_impute_draw_points", "dpmm_impute_draw_points_device"]
    binding = importlib.import_module(pkg.__name__ + ".binding")
    assert sorted(n for n, _, _ in binding.ABI_IMPUTE) == declared
    others = (binding.ABI + binding.ABI_TENSOR + binding.ABI_SCORE + binding.ABI_RANK + binding.ABI_OVERLAP + binding.ABI_TRACE + binding.ABI_MISSING + binding.ABI_CSC
              + binding.ABI_SAMPLE + binding.ABI_PROJECT)
    assert not set(declared) & set(n for n, _, _ in others)
    for n, _, args in binding.ABI_IMPUTE:                                 # ctx, out, ld, draw_stride, comp, seed, i0, draw0, ndraws
        assert len(args) == 9 and args[5] is ctypes.c_uint64 and args[2:4] == [ctypes.c_int64] * 2 and args[6:] == [ctypes.c_int64] * 3
    assert int(re.search(r"#define DPMM_IMPUTE_MAX_DRAWS (\d+)", hdr).group(1)) == binding.IMPUTE_MAX_DRAWS == 1 << 26
    dev = open(os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc", "dpmm_device.h")).read()
    streams = {k: int(v) for k, v in re.findall(r"\b(STREAM_[A-Z_]+) = (\d+)", dev)}
    assert (streams["STREAM_IMPUTE_COMP"], streams["STREAM_IMPUTE_NORMAL"], streams["STREAM_IMPUTE_CHI"]) == (ir.STREAM_COMP, ir.STREAM_NORMAL, ir.STREAM_CHI)
    assert len(set(streams.values())) == len(streams) and all(f"stream {v}" in hdr for v in (43, 44, 45))
    mk = open(os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "build/missing.o" in objs and re.search(r"^build/dpmm_api\.o:.*dpmm_hip_impute\.h", mk, flags=re.M)
    assert re.search(r"^build/%\.o:.*sample_device\.h", mk, flags=re.M)
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for n in declared:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                                   # additive: the version stays
    assert callable(binding.Worker.impute_draws_into)
