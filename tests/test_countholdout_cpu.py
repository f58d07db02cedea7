"""CPU-side checks of the held-out count points and of Multinomial model growth (include/dpmm_hip_countholdout.h, host/score.py:
Predictor.held_out_counts / grow_counts, host/absorb.py: dirichlet_graft): the header compiles as C, its functions are bound, exported and
built from csrc/holdout.hip with the shared class function; `dirichlet_graft` by hand; the numpy class rule of
tests/tools/countholdout_ref.py on hand-made points; the prior's alpha through `save` / `load`; the argument checks over a stand-in worker
(tests/fake_worker.py, subclassed here) whose rule is "the first feature exceeds 100"."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from __graft_entry__ import ROOT, load_package
from tools import countholdout_ref as R

HEADER = os.path.join(ROOT, "include", "dpmm_hip_countholdout.h")
FUNCS = ["dpmm_countholdout_accumulate", "dpmm_countholdout_begin", "dpmm_countholdout_read", "dpmm_countstats_set_per_count"]


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
def test_header_compiles_as_c_and_is_bound_exported_and_built(pkg, host):
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER])
    body = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", body))) == FUNCS
    binding = importlib.import_module(pkg.__name__ + ".binding")
    abi = {n: (res, args) for n, res, args in binding.ABI_COUNTHOLDOUT}
    assert sorted(abi) == FUNCS
    ctype = {"dpmm_ctx *": ctypes.c_void_p, "int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64,
             "const dpmm_countholdout_dst *": ctypes.POINTER(binding.CountHoldoutDst), "const dpmm_countholdout_out *": ctypes.POINTER(binding.CountHoldoutOut)}
    for name in FUNCS:
        ret, params = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", body).groups()
        types_ = [re.sub(r"\s*\w+$", "", p.strip()).strip() for p in params.split(",")]
        assert ret == "int" and abi[name][0] is ctypes.c_int
        assert [ctype[t] for t in types_] == abi[name][1], (name, types_)
    dst = body[body.index("typedef struct {"):body.index("} dpmm_countholdout_dst;")]
    assert re.findall(r"\b([A-Za-z_]+);", dst) == [f[0] for f in binding.CountHoldoutDst._fields_]
    out = body[body.index("} dpmm_countholdout_dst;"):body.index("} dpmm_countholdout_out;")]
    assert re.findall(r"int64_t\s*\*\s*([A-Za-z_]+);", out) == [f[0] for f in binding.CountHoldoutOut._fields_]
    assert [f[0] for f in binding.CountHoldoutOut._fields_] == ["total", "total_entries", "stored", "stored_entries", "skipped", "incomplete", "scored"]
    for name in ("countstats_set_per_count", "countholdout_begin", "countholdout_accumulate", "countholdout_read"):
        assert callable(getattr(binding.Worker, name)), name
    csrc = os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "build/holdout.o" in re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "../../include/dpmm_hip_countholdout.h" in re.search(r"^build/dpmm_api\.o:(.*)$", mk, flags=re.M).group(1).split()
    hip = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "holdout.hip")).read())
    assert "cs_class(" in hip and "cs_mark_gaps(" in hip and "bs_table_passes(" in hip and '#include "countstats_device.h"' in hip
    assert "atomic" not in hip and "asm" not in hip and "__ballot(" in hip and "__popcll(" in hip
    assert "cs_class(" in re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "countstats.hip")).read())      # one rule, one piece of code
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for n in FUNCS:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                               # additive: the version stays
    for name in ("held_out_counts", "dirichlet_graft", "HeldOutCounts"):
        assert hasattr(host, name), name
    assert callable(host.Predictor.held_out_counts) and callable(host.Predictor.grow_counts)
    assert host.HeldOutCounts._fields == ("points", "index", "total", "total_entries", "skipped", "incomplete")


# ---------------------------------------------------------------------------------------------- dirichlet_graft
def test_dirichlet_graft_appends_in_float64_and_leaves_its_inputs_alone(host):
    rng = np.random.default_rng(1)
    K, Kn, D = 3, 2, 5
    old = dict(alpha=rng.uniform(0.5, 40.0, (K, D)))                 # Float64, as absorb_counts leaves it
    new = dict(alpha=rng.uniform(0.5, 4.0, (Kn, D)).astype(np.float32))
    count, ncount = np.array([40.0, 7.5, 3.0]), np.array([5, 6])
    before = old["alpha"].copy(), new["alpha"].copy(), count.copy(), ncount.copy()
    got, cnt = host.dirichlet_graft(old, count, new, ncount)
    assert got["alpha"].dtype == np.float64 and got["alpha"].shape == (K + Kn, D)
    assert got["alpha"][:K].tobytes() == old["alpha"].tobytes()     # the old rows: bit-equal
    assert np.array_equal(got["alpha"][K:], new["alpha"].astype(np.float64))
    assert not np.shares_memory(got["alpha"], old["alpha"]) and not np.shares_memory(got["alpha"], new["alpha"])
    assert cnt.dtype == np.float64 and cnt.tolist() == [40.0, 7.5, 3.0, 5.0, 6.0]
    assert old["alpha"].tobytes() == before[0].tobytes() and new["alpha"].tobytes() == before[1].tobytes()
    assert count.tobytes() == before[2].tobytes() and ncount.tobytes() == before[3].tobytes()
    got32, _ = host.dirichlet_graft(dict(alpha=old["alpha"].astype(np.float32)), count, new, ncount)      # Float32 rows keep their values
    assert got32["alpha"].dtype == np.float64 and np.array_equal(got32["alpha"][:K], old["alpha"].astype(np.float32).astype(np.float64))


def test_dirichlet_graft_refusals(host, pkg):
    binding = importlib.import_module(pkg.__name__ + ".binding")
    D = 4
    post, new = dict(alpha=np.ones((2, D))), dict(alpha=np.full((1, D), 2.0))
    host.dirichlet_graft(post, np.ones(2), new, np.ones(1))
    with pytest.raises(ValueError, match="features"):
        host.dirichlet_graft(post, np.ones(2), dict(alpha=np.ones((1, D + 1))), np.ones(1))
    with pytest.raises(ValueError, match="lacks 'alpha'"):
        host.dirichlet_graft(post, np.ones(2), dict(kappa=np.ones(1)), np.ones(1))
    with pytest.raises(ValueError, match="lacks 'alpha'"):
        host.dirichlet_graft(dict(m=np.ones((2, D))), np.ones(2), new, np.ones(1))
    with pytest.raises(ValueError, match=r"alpha \(K, D\)"):
        host.dirichlet_graft(post, np.ones(2), dict(alpha=np.ones(D)), np.ones(1))
    for bad in (np.nan, np.inf, -0.5):
        broken = dict(alpha=new["alpha"].copy())
        broken["alpha"][0, 1] = bad
        with pytest.raises(ValueError, match="not finite or is negative"):
            host.dirichlet_graft(post, np.ones(2), broken, np.ones(1))
    with pytest.raises(ValueError, match="one entry per cluster"):
        host.dirichlet_graft(post, np.ones(3), new, np.ones(1))
    with pytest.raises(ValueError, match="one entry per cluster"):
        host.dirichlet_graft(post, np.ones(2), new, np.ones(2))
    for bad in (np.nan, -1.0):
        with pytest.raises(ValueError, match="finite and non-negative"):
            host.dirichlet_graft(post, np.ones(2), new, np.array([bad]))
    assert binding.MAX_CLUSTERS == 1024
    with pytest.raises(ValueError, match="MAX_CLUSTERS"):                                     # 1024 + 1
        host.dirichlet_graft(dict(alpha=np.ones((binding.MAX_CLUSTERS, D))), np.ones(binding.MAX_CLUSTERS), new, np.ones(1))
    _, cnt = host.dirichlet_graft(dict(alpha=np.ones((binding.MAX_CLUSTERS - 1, D))), np.ones(binding.MAX_CLUSTERS - 1), new, np.ones(1))
    assert len(cnt) == binding.MAX_CLUSTERS


# ---------------------------------------------------------------------------------------------- the class rule, by hand
def test_class_rule_on_points_written_by_hand():
    #            0: ordinary   1: empty   2: NaN value   3: +Inf value   4: raw floor only   5: per count only   6: both   7: NaN score
    X = np.array([[4, 0, np.nan, 2, 50, 1, 30, 1],
                  [4, 0, 1, np.inf, 50, 1, 30, 1]], np.float32)
    ld = np.array([-8.0, -0.5, -3.0, -3.0, -120.0, -9.0, -400.0, np.nan], np.float32)
    f, fpc = -100.0, -4.0             # per count: -1, -inf (t = 0), -, -, -1.2, -4.5, -6.67
    c = R.classes(ld, X, f, fpc)
    assert c["t"].tolist() == [8.0, 0.0, 1.0, 2.0, 100.0, 2.0, 60.0, 2.0]
    assert c["complete"].tolist() == [True, True, False, False, True, True, True, True]
    assert c["skipped"].tolist() == [False] * 7 + [True]
    assert c["held"].tolist() == [False, False, False, False, True, True, True, False]
    assert c["incomplete"].tolist() == [False, False, True, True, False, False, False, False]       # never held out by the floor per count
    assert c["part"].tolist() == [True, True, False, False, False, False, False, False]             # the empty point takes part
    only = R.classes(ld, X, None, fpc)
    assert only["held"].tolist() == [False, False, False, False, False, True, True, False]
    raw = R.classes(ld, X, f, None)
    assert raw["held"].tolist() == [False, False, False, False, True, False, True, False]
    low = R.classes(np.array([-3.0, -3.0, -500.0, -500.0], np.float32), X[:, :4], -100.0, -1.0)        # the raw floor does hold an incomplete point out
    assert low["held"].tolist() == [False, False, True, True] and not low["incomplete"].any()
    # the sparse store: only stored entries count, an empty column has t = 0
    S = sp.csc_matrix((np.array([4, 4, np.nan, 1, 1, 1], np.float32), np.array([0, 1, 0, 1, 0, 1]), np.array([0, 2, 2, 4, 6])), shape=(2, 4))
    cs = R.classes(np.array([-8.0, -0.5, -3.0, -9.0], np.float32), S, None, -4.0)
    assert cs["t"].tolist() == [8.0, 0.0, 1.0, 2.0] and cs["held"].tolist() == [False, False, False, True] and cs["incomplete"].tolist() == [False, False, True, False]
    # the caps: the longest prefix inside both
    assert R.stored_prefix([3, 0, 5, 2], 10, 100) == (4, 10)
    assert R.stored_prefix([3, 0, 5, 2], 3, 100) == (3, 8)
    assert R.stored_prefix([3, 0, 5, 2], 10, 7) == (2, 3)           # the 5-entry point does not fit: it and everything behind it is dropped
    assert R.stored_prefix([3, 0, 5, 2], 10, 8) == (3, 8)
    assert R.stored_prefix([3, 0, 5, 2], 0, 100) == (0, 0) and R.stored_prefix([], 5, 5) == (0, 0)


# ---------------------------------------------------------------------------------------------- a stand-in worker
def stand_in():
    from fake_worker import FakeWorker

    class CountHoldWorker(FakeWorker):
        """Takes the predictive parameters, keeps the last upload and holds out the points whose first feature exceeds 100."""
        holdout_device = "cpu"
        loads, begun = [], 0

        def set_predictive_mult(self, logp, weights):
            CountHoldWorker.loads.append(len(weights))

        def set_predictive_niw(self, *a):
            pass

        def countholdout_begin(self, dst, min_logdens=None, min_logdens_per_count=None):
            CountHoldWorker.begun += 1
            self._dst, self._cnt = dst, dict(total=0, skipped=0, incomplete=0, scored=0)

        def countholdout_accumulate(self, lo, n_valid):
            import torch
            X = self.X[:n_valid]
            for i in np.flatnonzero(X[:, 0] > 100):
                s = self._cnt["total"]
                if s < self._dst["cap"]:
                    self._dst["points"][s] = torch.from_numpy(X[i])
                    self._dst["index"][s] = lo + int(i)
                self._cnt["total"] += 1
            self._cnt["scored"] += int((X[:, 0] <= 100).sum())

        def countholdout_read(self):
            st = min(self._cnt["total"], self._dst["cap"])
            return dict(self._cnt, stored=st, total_entries=self._cnt["total"] * self.D, stored_entries=st * self.D)
    CountHoldWorker.loads, CountHoldWorker.begun = [], 0
    return CountHoldWorker


def predictor(score, D, K, factory, prior=True, kind=1, capacity=16):
    p = score.Predictor.__new__(score.Predictor)
    if kind == 1:
        post = dict(alpha=np.ones((K, D), np.float32) + np.eye(K, D, dtype=np.float32))
        p._setup(1, D, 10.0, np.full(K, 50.0), post, capacity, 0, factory, prior_alpha=np.full(D, 0.5) if prior else None)
    else:
        post = dict(kappa=np.ones(K), nu=np.full(K, D + 3.0), m=np.zeros((K, D)), U=np.tile(np.eye(D) * np.sqrt(D + 3.0), (K, 1, 1)), logdet_psi=np.zeros(K))
        p._setup(0, D, 10.0, np.full(K, 50.0), post, capacity, 0, factory)
    return p


def batch(D, n, far):
    X = np.random.default_rng(8).integers(0, 5, (D, n)).astype(np.float32)
    X[0, far] = 500.0
    return X


def test_held_out_counts_walks_the_slabs_and_validates_its_arguments(score, host):
    Worker = stand_in()
    D, K, n = 3, 2, 37                                               # capacity 16: two full slabs and a short one
    far = [0, 15, 16, 31, 32, 36]
    X = batch(D, n, far)
    p = predictor(score, D, K, Worker)
    h = p.held_out_counts(X, min_logdens_per_count=-3.0)
    assert isinstance(h, host.HeldOutCounts) and isinstance(h.points, np.ndarray) and h.points.shape == (D, len(far)) and h.points.dtype == np.float32
    assert h.index.dtype == np.int64 and h.index.tolist() == far and np.array_equal(h.points, X[:, far])
    assert (h.total, h.total_entries) == (len(far), len(far) * D)
    h = p.held_out_counts(X, min_logdens=-50.0, max_points=4)
    assert h.index.tolist() == far[:4] and h.total == len(far) and h.points.shape == (D, 4)
    h = p.held_out_counts(X, min_logdens=-50.0, max_entries=2 * D + 1)        # dense: cap = max_entries // D
    assert h.index.tolist() == far[:2] and h.total == len(far)
    h = p.held_out_counts(X, min_logdens=-50.0, max_points=0)                 # count only
    assert h.points.shape == (D, 0) and h.index.shape == (0,) and h.total == len(far)
    begun = Worker.begun
    for call in (p.held_out_counts, p.grow_counts):
        with pytest.raises(ValueError, match="needs a floor"):
            call(X)
        with pytest.raises(ValueError, match="min_logdens_per_count must not be NaN"):
            call(X, min_logdens_per_count=float("nan"))
        with pytest.raises(ValueError, match="min_logdens must not be NaN"):
            call(X, min_logdens=float("nan"))
        with pytest.raises(ValueError, match="max_points"):
            call(X, min_logdens=-5.0, max_points=-1)
        with pytest.raises(ValueError, match="max_entries"):
            call(X, min_logdens=-5.0, max_entries=-1)
        with pytest.raises(ValueError, match="dimension"):
            call(X[:2], min_logdens=-5.0)
    with pytest.raises(ValueError, match="min_points"):
        p.grow_counts(X, min_logdens=-5.0, min_points=0)
    with pytest.raises(ValueError, match="alpha"):
        p.grow_counts(X, min_logdens=-5.0, alpha=0.0)
    with pytest.raises(ValueError, match="multinomial_hyper over"):
        p.grow_counts(X, min_logdens=-5.0, prior=host.multinomial_hyper(np.ones(D + 1)))
    with pytest.raises(ValueError, match="multinomial_hyper over"):
        p.grow_counts(X, min_logdens=-5.0, prior=host.niw_hyperparams(1.0, np.zeros(D), D + 3, np.eye(D)))
    bare = predictor(score, D, K, Worker, prior=False)                # a missing prior_alpha
    with pytest.raises(ValueError, match="prior_alpha.*prior="):
        bare.grow_counts(X, min_logdens=-5.0)
    assert Worker.begun == begun                                     # every refusal came before the worker was asked for anything
    niw = predictor(score, D, K, Worker, kind=0)                      # an NIW model
    with pytest.raises(ValueError, match="Multinomial prior: an NIW model has held_out"):
        niw.held_out_counts(X, min_logdens=-5.0)
    with pytest.raises(ValueError, match="Multinomial prior: an NIW model has grow"):
        niw.grow_counts(X, min_logdens=-5.0)
    with pytest.raises(ValueError, match="count_statistics are for the Multinomial prior"):
        niw.count_statistics(X, min_logdens_per_count=-1.0)
    with pytest.raises(ValueError, match="min_logdens_per_count must not be NaN"):
        p.count_statistics(X, min_logdens_per_count=float("nan"))
    with pytest.raises(RuntimeError, match="dpmm_countstats_begin"):                          # the stand-in has no count statistics at all
        p.count_statistics(X, min_logdens_per_count=-1.0)
    assert Worker.begun == begun
    from fake_worker import FakeWorker
    plain = predictor(score, D, K, type("Bare", (FakeWorker,), {"set_predictive_mult": lambda self, *a: None}))
    with pytest.raises(RuntimeError, match="dpmm_countholdout_begin"):
        plain.held_out_counts(X, min_logdens=-5.0)
    for x in (bare, niw, plain):
        x.close()
    p.close()
    for call in (p.held_out_counts, p.grow_counts):
        with pytest.raises(RuntimeError, match="closed"):
            call(X, min_logdens=-5.0)


def test_save_and_load_carry_prior_alpha_and_a_file_without_it_still_loads(score, host, tmp_path):
    Worker = stand_in()
    D, K = 3, 2
    p = predictor(score, D, K, Worker)
    assert p.prior_alpha.dtype == np.float64 and p.prior_alpha.tolist() == [0.5] * D and p.prior_hyper is None
    path = str(tmp_path / "with.npz")
    p.save(path)
    with np.load(path) as z:
        assert "prior_alpha" in z.files and z["prior_alpha"].tolist() == [0.5] * D
        old = {k: z[k] for k in z.files if k != "prior_alpha"}
    q = score.Predictor.load(path, worker_factory=Worker, capacity=16)
    assert q.prior_alpha.dtype == np.float64 and np.array_equal(q.prior_alpha, p.prior_alpha) and q.kind == 1
    assert q.post["alpha"].tobytes() == p.post["alpha"].tobytes()
    bare = str(tmp_path / "without.npz")
    np.savez(bare, **old)                                            # a model file written before the prior was kept
    r = score.Predictor.load(bare, worker_factory=Worker, capacity=16)
    assert r.prior_alpha is None and r.K == K
    X = batch(D, 20, [3, 17])
    with pytest.raises(ValueError, match="prior_alpha.*prior="):
        r.grow_counts(X, min_logdens=-5.0)
    called = []

    def fit(points, prior, alpha, **kw):
        called.append((points, prior, alpha, kw))
        raise RuntimeError("stop here")
    api = importlib.import_module(score.__name__.rsplit(".", 1)[0] + ".api")
    orig, api.fit = api.fit, fit
    snap = r.post["alpha"].tobytes(), r.points_count.tobytes(), r.weights.tobytes(), r.K
    try:
        with pytest.raises(RuntimeError, match="stop here"):        # with prior= the same Predictor goes on to the sub-fit
            r.grow_counts(X, min_logdens=-5.0, prior=host.multinomial_hyper(np.full(D, 2.0)), iters=7, seed=5)
    finally:
        api.fit = orig
    assert len(called) == 1 and called[0][1].alpha.tolist() == [2.0] * D and called[0][2] == r.alpha
    assert called[0][3] == dict(iters=7, seed=5, verbose=False)
    pts = called[0][0]                                               # the captured tensor where it lies: (D, 2), point-major memory
    assert tuple(pts.shape) == (D, 2) and pts.T.is_contiguous() and np.array_equal(pts.numpy(), X[:, [3, 17]])
    assert (r.post["alpha"].tobytes(), r.points_count.tobytes(), r.weights.tobytes(), r.K) == snap      # a failure leaves the Predictor as it was
    # a model object whose prior is a multinomial_hyper hands its alpha to the Predictor
    import types
    s = types.SimpleNamespace(K=K, prior=host.multinomial_hyper(np.arange(1.0, D + 1)), alpha=10.0, points_count=np.full(K, 9),
                              post=dict(alpha=np.ones((3 * K, D), np.float32)), wk=types.SimpleNamespace(device=0))
    m = score.Predictor(types.SimpleNamespace(sampler=s), capacity=16, worker_factory=Worker)
    assert m.prior_alpha.tolist() == [1.0, 2.0, 3.0]
    for x in (p, q, r, m):
        x.close()
