"""CPU-side checks of the held-out points and of model growth (include/dpmm_hip_holdout.h, host/score.py: Predictor.held_out / grow,
host/absorb.py: niw_graft): the header compiles as C, its functions are bound, exported, built from csrc/holdout.hip and match the Julia
stub; `niw_graft` by hand; the prior's hyper-parameters through `save` / `load`; the argument checks and the all-or-nothing update of
`grow` over a stand-in worker (tests/fake_worker.py, subclassed here) whose rule is "the first feature exceeds 100"."""
import ctypes
import importlib
import os
import re
import subprocess
import types

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package

HEADER = os.path.join(ROOT, "include", "dpmm_hip_holdout.h")
FUNCS = ["dpmm_holdout_accumulate", "dpmm_holdout_begin", "dpmm_holdout_read"]
POST_KEYS = ("kappa", "nu", "m", "U", "logdet_psi")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


@pytest.fixture(scope="module")
def host(pkg):
    return importlib.import_module(pkg.__name__ + ".host")


# ---------------------------------------------------------------------------------------------- the C boundary
def test_header_compiles_as_c_and_is_bound_exported_built_and_matches_the_julia_stub(pkg, host):
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER])
    body = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", body))) == FUNCS
    binding = importlib.import_module(pkg.__name__ + ".binding")
    abi = {n: (res, args) for n, res, args in binding.ABI_HOLDOUT}
    assert sorted(abi) == FUNCS
    others = (binding.ABI + binding.ABI_TENSOR + binding.ABI_SCORE + binding.ABI_RANK + binding.ABI_OVERLAP + binding.ABI_BATCHSTATS + binding.ABI_COUNTSTATS
              + binding.ABI_TYPICALITY + binding.ABI_TRACE + binding.ABI_MISSING + binding.ABI_IMPUTE + binding.ABI_CSC + binding.ABI_SAMPLE + binding.ABI_PROJECT)
    assert not set(FUNCS) & set(n for n, _, _ in others)
    # the argument lists of the header, type by type
    ctype = {"dpmm_ctx *": ctypes.c_void_p, "int": ctypes.c_int, "float": ctypes.c_float, "float *": ctypes.c_void_p, "int64_t *": ctypes.c_void_p,
             "int64_t": ctypes.c_int64, "const dpmm_holdout_out *": ctypes.POINTER(binding.HoldoutOut)}
    for name in FUNCS:
        ret, params = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", body).groups()
        types_ = [re.sub(r"\s*\w+$", "", p.strip()).strip() for p in params.split(",")]
        assert ret == "int" and abi[name][0] is ctypes.c_int
        assert [ctype[t] for t in types_] == abi[name][1], (name, types_)
    struct = body[body.index("typedef struct {"):body.index("} dpmm_holdout_out;")]
    fields = re.findall(r"int64_t\s*\*\s*([A-Za-z_]+);", struct)
    assert fields == [f[0] for f in binding.HoldoutOut._fields_] == ["total", "stored", "skipped", "incomplete", "scored"]
    for name in ("holdout_begin", "holdout_accumulate", "holdout_read"):
        assert callable(getattr(binding.Worker, name)), name
    # the Julia stub: the same functions, the same fields in the same order, the same argument types
    jl = open(os.path.join(ROOT, "julia", "gpu_holdout.jl")).read()
    assert set(re.findall(r":(dpmm_[a-z0-9_]+)", jl)) == set(FUNCS)
    jstruct = jl[jl.index("struct DpmmHoldoutOut"):jl.index("end", jl.index("struct DpmmHoldoutOut"))]
    assert re.findall(r"(\w+)::Ptr\{Int64\}", jstruct) == fields
    jtype = {ctypes.c_int: "Cint", ctypes.c_float: "Cfloat", ctypes.c_int64: "Int64"}
    for name in FUNCS:
        sig = re.search(r":" + name + r", libdpmm\), Cint, \(([^)]*)\)", jl).group(1)
        got = [t.strip() for t in sig.split(",") if t.strip()]
        assert len(got) == len(abi[name][1]), name
        for j, c in zip(got, abi[name][1]):
            assert j == jtype[c] if c in jtype else (j.startswith("Ptr{") or j.startswith("Ref{")), (name, j, c)
    # built from csrc/holdout.hip with the shared classification, no atomics
    csrc = os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "build/holdout.o" in re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "../../include/dpmm_hip_holdout.h" in re.search(r"^build/dpmm_api\.o:(.*)$", mk, flags=re.M).group(1).split()
    hip = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "holdout.hip")).read())
    assert "bs_class(" in hip and "bs_table_passes(" in hip and "bs_mark_gaps(" in hip and '#include "batchstats_device.h"' in hip
    assert "atomic" not in hip and "asm" not in hip and "__ballot(" in hip and "__popcll(" in hip
    assert "bs_class(" in re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "batchstats.hip")).read())      # one rule, one piece of code
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for n in FUNCS:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                               # additive: the version stays
    assert callable(host.held_out) and callable(host.Predictor.held_out) and callable(host.Predictor.grow) and callable(host.niw_graft)
    assert host.HeldOut._fields == ("points", "index", "total", "skipped", "incomplete")
    assert host.Growth._fields == ("added", "sizes", "index", "labels", "dropped", "total", "model")


# ---------------------------------------------------------------------------------------------- niw_graft
def posteriors(D, K, seed, dtype=np.float64):
    """K NIW posteriors around means 20 k e_0 with psi = I: U U' = nu psi, logdet_psi = 0."""
    rng = np.random.default_rng(seed)
    nu = rng.uniform(D + 5, D + 50, K)
    m = rng.normal(size=(K, D))
    m[:, 0] += 20.0 * np.arange(K)
    U = np.sqrt(nu)[:, None, None] * np.eye(D)[None]
    return {"kappa": rng.uniform(5, 50, K).astype(dtype), "nu": nu.astype(dtype), "m": m.astype(dtype), "U": U.astype(dtype),
            "logdet_psi": np.zeros(K, dtype)}


def test_niw_graft_appends_in_float64_and_leaves_its_inputs_alone(host):
    D, K, Kn = 3, 2, 3
    post, new = posteriors(D, K, 1), posteriors(D, Kn, 2, np.float32)
    count, ncount = np.array([40.0, 7.5]), np.array([5, 6, 7])
    before = {k: v.copy() for k, v in post.items()}, {k: v.copy() for k, v in new.items()}, count.copy(), ncount.copy()
    got, cnt = host.niw_graft(post, count, new, ncount)
    for k in POST_KEYS:
        assert got[k].dtype == np.float64 and got[k].shape == (K + Kn,) + post[k].shape[1:], k
        assert got[k][:K].tobytes() == post[k].tobytes(), k                                   # the old rows: bit-equal
        assert np.array_equal(got[k][K:], new[k].astype(np.float64)), k
        assert post[k].tobytes() == before[0][k].tobytes() and new[k].tobytes() == before[1][k].tobytes(), k
        assert not np.shares_memory(got[k], post[k]) and not np.shares_memory(got[k], new[k])
    assert cnt.dtype == np.float64 and cnt.tolist() == [40.0, 7.5, 5.0, 6.0, 7.0]
    assert count.tobytes() == before[2].tobytes() and ncount.tobytes() == before[3].tobytes()


def test_niw_graft_refusals(host, pkg):
    binding = importlib.import_module(pkg.__name__ + ".binding")
    D = 2
    post, new = posteriors(D, 2, 3), posteriors(D, 1, 4)
    ok = (post, np.ones(2), new, np.ones(1))
    host.niw_graft(*ok)
    with pytest.raises(ValueError, match="features"):
        host.niw_graft(post, np.ones(2), posteriors(D + 1, 1, 4), np.ones(1))
    with pytest.raises(ValueError, match="one entry per cluster"):
        host.niw_graft(post, np.ones(3), new, np.ones(1))
    with pytest.raises(ValueError, match="one entry per cluster"):
        host.niw_graft(post, np.ones(2), new, np.ones(2))
    with pytest.raises(ValueError, match="lacks"):
        host.niw_graft(post, np.ones(2), {k: v for k, v in new.items() if k != "U"}, np.ones(1))
    with pytest.raises(ValueError, match="must hold"):
        host.niw_graft(post, np.ones(2), dict(new, U=new["U"][:, :1]), np.ones(1))
    for key in POST_KEYS:
        for bad in (np.nan, np.inf):
            broken = {k: v.copy() for k, v in new.items()}
            broken[key].flat[0] = bad
            with pytest.raises(ValueError, match="not finite"):
                host.niw_graft(post, np.ones(2), broken, np.ones(1))
    with pytest.raises(ValueError, match="finite and non-negative"):
        host.niw_graft(post, np.ones(2), new, np.array([np.nan]))
    with pytest.raises(ValueError, match="finite and non-negative"):
        host.niw_graft(post, np.ones(2), new, np.array([-1.0]))
    assert binding.MAX_CLUSTERS == 1024
    big = posteriors(D, binding.MAX_CLUSTERS, 5)
    with pytest.raises(ValueError, match="MAX_CLUSTERS"):                                     # 1024 + 1
        host.niw_graft(big, np.ones(binding.MAX_CLUSTERS), new, np.ones(1))
    got, cnt = host.niw_graft(posteriors(D, binding.MAX_CLUSTERS - 1, 6), np.ones(binding.MAX_CLUSTERS - 1), new, np.ones(1))      # 1023 + 1 fits
    assert len(cnt) == binding.MAX_CLUSTERS


# ---------------------------------------------------------------------------------------------- a stand-in worker
def stand_in():
    from fake_worker import FakeWorker

    class HoldWorker(FakeWorker):
        """Takes the predictive parameters, keeps the last upload and holds out the points whose first feature exceeds 100."""
        holdout_device = "cpu"
        loads = []          # K of every set_predictive_niw
        begun = 0

        def set_predictive_niw(self, m, R, logdet, df, weights):
            HoldWorker.loads.append(len(weights))

        def set_predictive_mult(self, *a):
            pass

        def holdout_begin(self, dst_points, dst_index, cap, min_logdens=None, min_tail=None):
            HoldWorker.begun += 1
            self._dst, self._cap, self._cnt = (dst_points, dst_index), int(cap), dict(total=0, stored=0, skipped=0, incomplete=0, scored=0)

        def holdout_accumulate(self, lo, n_valid):
            import torch
            X = self.X[:n_valid]
            for i in np.flatnonzero(X[:, 0] > 100):
                s = self._cnt["total"]
                if s < self._cap:
                    self._dst[0][s] = torch.from_numpy(X[i])
                    self._dst[1][s] = lo + int(i)
                self._cnt["total"] += 1
            self._cnt["scored"] += int((X[:, 0] <= 100).sum())

        def holdout_read(self):
            return dict(self._cnt, stored=min(self._cnt["total"], self._cap))
    HoldWorker.loads, HoldWorker.begun = [], 0
    return HoldWorker


def predictor(score, D, K, factory, hyper=True, capacity=16):
    p = score.Predictor.__new__(score.Predictor)
    prior = dict(kappa=1.0, m=np.zeros(D), nu=D + 3.0, psi=np.eye(D)) if hyper else None
    p._setup(0, D, 10.0, np.full(K, 50.0), posteriors(D, K, 3), capacity, 0, factory, prior_hyper=prior)
    return p


def batch(D, n, far):
    X = np.random.default_rng(8).normal(size=(D, n)).astype(np.float32)
    X[0, far] = 500.0
    return X


# ---------------------------------------------------------------------------------------------- save / load carry the prior
def test_save_and_load_carry_the_prior_and_a_file_without_it_still_loads(score, host, tmp_path):
    Worker = stand_in()
    D, K = 3, 2
    p = predictor(score, D, K, Worker)
    assert p.prior_hyper["m"].dtype == np.float64 and p.prior_hyper["psi"].shape == (D, D)
    path = str(tmp_path / "with.npz")
    p.save(path)
    with np.load(path) as z:
        assert {"prior_kappa", "prior_m", "prior_nu", "prior_psi"} <= set(z.files)
        assert float(z["prior_kappa"]) == 1.0 and float(z["prior_nu"]) == D + 3.0 and np.array_equal(z["prior_psi"], np.eye(D))
        old = {k: z[k] for k in z.files if not k.startswith("prior_")}
    q = score.Predictor.load(path, worker_factory=Worker, capacity=16)
    for k in ("kappa", "m", "nu", "psi"):
        assert np.array_equal(q.prior_hyper[k], p.prior_hyper[k]) and q.prior_hyper[k].dtype == np.float64, k
    bare = str(tmp_path / "without.npz")
    np.savez(bare, **old)                                            # a model file written before the prior was kept
    r = score.Predictor.load(bare, worker_factory=Worker, capacity=16)
    assert r.prior_hyper is None and r.K == K
    for k in POST_KEYS:
        assert r.post[k].tobytes() == p.post[k].tobytes(), k
    X = batch(D, 20, [3, 17])
    with pytest.raises(ValueError, match="hyper-parameters.*prior="):
        r.grow(X, min_tail=1e-4)
    assert Worker.begun == 0
    called = []

    def fit(points, prior, alpha, **kw):
        called.append((prior, alpha, kw))
        raise RuntimeError("stop here")
    api = importlib.import_module(score.__name__.rsplit(".", 1)[0] + ".api")
    orig, api.fit = api.fit, fit
    try:
        with pytest.raises(RuntimeError, match="stop here"):        # with prior= the same Predictor goes on to the sub-fit
            r.grow(X, min_tail=1e-4, prior=host.niw_hyperparams(2.0, np.zeros(D), D + 4, np.eye(D)))
    finally:
        api.fit = orig
    assert len(called) == 1 and called[0][0].kappa == 2.0 and called[0][1] == r.alpha
    # a model object whose prior carries the hyper-parameters hands them to the Predictor; one without them leaves None
    s = types.SimpleNamespace(K=K, prior=host.niw_hyperparams(4.0, np.ones(D), D + 2, 2 * np.eye(D)), alpha=10.0, points_count=np.full(K, 9),
                              post={k: np.repeat(v, 3, axis=0) for k, v in posteriors(D, K, 3).items()}, wk=types.SimpleNamespace(device=0))
    m = score.Predictor(types.SimpleNamespace(sampler=s), capacity=16, worker_factory=Worker)
    assert float(m.prior_hyper["kappa"]) == 4.0 and np.array_equal(m.prior_hyper["psi"], 2 * np.eye(D))
    s.prior = types.SimpleNamespace(kind=0, dim=D)
    assert score.Predictor(types.SimpleNamespace(sampler=s), capacity=16, worker_factory=Worker).prior_hyper is None
    for x in (p, q, r, m):
        x.close()


# ---------------------------------------------------------------------------------------------- held_out / grow over the stand-in
def test_held_out_walks_the_slabs_and_validates_its_arguments(score, host):
    Worker = stand_in()
    D, K, n = 3, 2, 37                                               # capacity 16: two full slabs and a short one
    far = [0, 15, 16, 31, 32, 36]
    X = batch(D, n, far)
    p = predictor(score, D, K, Worker)
    h = p.held_out(X, min_tail=1e-3)
    assert isinstance(h, host.HeldOut) and isinstance(h.points, np.ndarray) and h.points.shape == (D, len(far)) and h.points.dtype == np.float32
    assert h.index.dtype == np.int64 and h.index.tolist() == far and np.array_equal(h.points, X[:, far]) and h.total == len(far)
    h = p.held_out(X, min_logdens=-50.0, max_points=4)
    assert h.index.tolist() == far[:4] and h.total == len(far) and h.points.shape == (D, 4)
    h = p.held_out(X[:, 1:15], min_tail=0.5)
    assert h.points.shape == (D, 0) and h.index.shape == (0,) and h.total == 0
    begun = Worker.begun
    for call in (p.held_out, p.grow):
        with pytest.raises(ValueError, match="needs a floor"):
            call(X)
        for bad in (0.0, -0.1, 1.0000001, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="min_tail"):
                call(X, min_tail=bad)
        with pytest.raises(ValueError, match="min_logdens"):
            call(X, min_logdens=float("nan"))
        with pytest.raises(ValueError, match="max_points"):
            call(X, min_tail=0.5, max_points=-1)
        with pytest.raises(ValueError, match="dimension"):
            call(X[:2], min_tail=0.5)
    with pytest.raises(ValueError, match="min_points"):
        p.grow(X, min_tail=0.5, min_points=0)
    with pytest.raises(ValueError, match="alpha"):
        p.grow(X, min_tail=0.5, alpha=0.0)
    with pytest.raises(ValueError, match="niw_hyperparams over"):
        p.grow(X, min_tail=0.5, prior=host.niw_hyperparams(1.0, np.zeros(D + 1), D + 4, np.eye(D + 1)))
    assert Worker.begun == begun                                     # every refusal came before the worker was asked for anything
    mult = score.Predictor.__new__(score.Predictor)
    mult._setup(1, D, 10.0, np.full(K, 5.0), dict(alpha=np.ones((K, D), np.float32)), 16, 0, Worker)
    for call in (mult.held_out, mult.grow):
        with pytest.raises(ValueError, match="NIW.*Multinomial.*out of scope"):
            call(X, min_tail=0.5)
    mult.close()
    from fake_worker import FakeWorker
    bare = predictor(score, D, K, type("Bare", (FakeWorker,), {"set_predictive_niw": lambda self, *a: None}))
    with pytest.raises(RuntimeError, match="dpmm_holdout_begin"):
        bare.held_out(X, min_tail=0.5)
    bare.close()
    p.close()
    for call in (p.held_out, p.grow):
        with pytest.raises(RuntimeError, match="closed"):
            call(X, min_tail=0.5)


def snapshot(p):
    return {k: v.tobytes() for k, v in p.post.items()}, p.points_count.tobytes(), p.weights.tobytes(), p.K


def test_grow_is_all_or_nothing_and_appends_what_the_sub_fit_found(score, host):
    Worker = stand_in()
    D, K, n = 3, 2, 40
    far = list(range(5, 17))                                         # 12 points across the first slab boundary
    X = batch(D, n, far)
    p = predictor(score, D, K, Worker)
    p._sampler_set = True
    before, loads = snapshot(p), list(Worker.loads)
    api = importlib.import_module(score.__name__.rsplit(".", 1)[0] + ".api")
    orig = api.fit
    seen = {}

    def failing(points, prior, alpha, **kw):
        seen.update(points=points, prior=prior, alpha=alpha, kw=kw)
        raise RuntimeError("the sub-fit failed")

    sub = posteriors(D, 2, 9)
    lab = np.array([1] * 9 + [2] * 3)                                # sub-cluster 2 is smaller than min_points = D + 1

    def working(points, prior, alpha, **kw):
        s = types.SimpleNamespace(K=2, post={k: np.repeat(v, 3, axis=0) for k, v in sub.items()})
        model = types.SimpleNamespace(sampler=s)
        return (lab, None, None, 0, None, None, None, None, model)

    def broken(points, prior, alpha, **kw):                         # a sub-model niw_graft refuses: the kept cluster's kappa is NaN
        res = working(points, prior, alpha, **kw)
        res[8].sampler.post["kappa"][0] = np.nan
        return res
    try:
        api.fit = failing
        with pytest.raises(RuntimeError, match="sub-fit failed"):
            p.grow(X, min_tail=1e-4, iters=7, seed=5, burnout=2)
        assert snapshot(p) == before and Worker.loads == loads and p._sampler_set
        pts = seen["points"]                                         # the captured tensor where it lies: (D, 12), point-major memory
        assert tuple(pts.shape) == (D, len(far)) and pts.T.is_contiguous() and np.array_equal(pts.numpy(), X[:, far])
        assert seen["alpha"] == p.alpha and seen["prior"].kappa == 1.0 and seen["prior"].nu == D + 3.0
        assert seen["kw"] == dict(iters=7, seed=5, verbose=False, burnout=2)
        api.fit = broken
        with pytest.raises(ValueError, match="not finite"):
            p.grow(X, min_tail=1e-4)
        assert snapshot(p) == before and Worker.loads == loads and p._sampler_set
        api.fit = working
        g = p.grow(X, min_tail=1e-4, min_points=10)                  # no sub-cluster is large enough
        assert (g.added, g.dropped, g.total) == (0, 12, 12) and len(g.index) == len(g.labels) == len(g.sizes) == 0
        assert snapshot(p) == before and Worker.loads == loads and p._sampler_set
        g = p.grow(X[:, :5], min_tail=1e-4)                          # nothing held out: no sub-fit, nothing changes
        assert (g.added, g.dropped, g.total, g.model) == (0, 0, 0, None) and snapshot(p) == before and Worker.loads == loads
        g = p.grow(X, min_tail=1e-4)
    finally:
        api.fit = orig
    assert isinstance(g, host.Growth) and (g.added, g.dropped, g.total) == (1, 3, 12) and g.sizes.tolist() == [9]
    assert g.index.tolist() == far[:9] and g.labels.tolist() == [3] * 9 and g.index.dtype == g.labels.dtype == np.int64
    assert p.K == 3 and Worker.loads == loads + [3] and not p._sampler_set          # ONE reload, with the new K
    for k in POST_KEYS:
        assert p.post[k][:K].tobytes() == before[0][k] and p.post[k][K:].tobytes() == sub[k][:1].tobytes(), k
    assert p.points_count[:K].tobytes() == before[1] and p.points_count[K] == 9.0
    w = p.points_count + p.alpha
    assert p.weights.dtype == np.float32 and np.array_equal(p.weights, (w / w.sum()).astype(np.float32))
    p.close()
