"""CPU-side checks of exemplars (include/dpmm_hip_rank.h): the header compiles as C, its functions are bound, exported and built from
csrc/rank.hip; `Predictor.exemplars` walks the slabs of `_run` over a stand-in worker that keeps a numpy table, and equals the
definitions (tests/tools/rank_ref.py) whatever the capacity; the refusals."""
import ctypes
import importlib
import os
import re
import subprocess
import types

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package
from fake_worker import FakeWorker
from tools import rank_ref

HEADER = os.path.join(ROOT, "include", "dpmm_hip_rank.h")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


# ---------------------------------------------------------------------------------------------- the C boundary
def test_header_compiles_as_c_and_is_bound_exported_and_built(pkg):
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER])
    hdr = open(HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", body)))
    assert declared == ["dpmm_rank_accumulate", "dpmm_rank_begin", "dpmm_rank_read", "dpmm_rank_read_device"]
    binding = importlib.import_module(pkg.__name__ + ".binding")
    assert sorted(n for n, _, _ in binding.ABI_RANK) == declared
    assert not set(declared) & set(n for n, _, _ in binding.ABI + binding.ABI_TENSOR + binding.ABI_SCORE + binding.ABI_CSC + binding.ABI_SAMPLE)
    for name in ("rank_begin", "rank_accumulate", "rank_read"):
        assert callable(getattr(binding.Worker, name)), name
    assert int(re.search(r"#define DPMM_RANK_MAX_M (\d+)", hdr).group(1)) == binding.RANK_MAX_M == 64
    assert int(re.search(r"#define DPMM_RANK_TYPICAL (\d+)", hdr).group(1)) == binding.RANK_TYPICAL == 1
    assert int(re.search(r"#define DPMM_RANK_FRINGE (\d+)", hdr).group(1)) == binding.RANK_FRINGE == 2
    struct = body[body.index("typedef struct {"):body.index("} dpmm_rank_out;")]
    assert re.findall(r"\*\s*([a-z_]+);", struct) == [f[0] for f in binding.RankOut._fields_]
    mk = open(os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "build/rank.o" in objs and "dpmm_hip_rank.h" in mk
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for n in declared:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                               # additive: the version stays
    host = importlib.import_module(pkg.__name__ + ".host")
    assert callable(host.exemplars) and callable(host.Predictor.exemplars)


# ---------------------------------------------------------------------------------------------- the reference itself
def test_rank_ref_on_a_table_written_by_hand():
    nan, inf = np.nan, np.inf
    #                 0    1    2    3     4     5    6    7
    tab = np.array([[1.0, 5.0, 2.0, nan, -inf, 7.0, 7.0, 0.5],
                    [3.0, 5.0, 9.0, 8.0, -inf, 1.0, 1.0, inf]], np.float32)
    lab, s, part = rank_ref.labels_and_scores(tab)
    assert list(lab) == [2, 1, 2, 1, 1, 1, 1, 2]                   # point 1: the first maximum; point 3: the first NaN
    assert list(part) == [True, True, True, False, False, True, True, False]
    r = rank_ref.rank(tab, 2, index_base=100)
    assert r["skipped"] == 3 and list(r["count"]) == [3, 2]
    assert r["typ_idx"].tolist() == [[105, 106], [102, 100]] and r["typ_score"].tolist() == [[7.0, 7.0], [9.0, 3.0]]      # the tie: lower index first
    assert r["fringe_idx"].tolist() == [[101, 105], [100, 102]] and r["fringe_score"].tolist() == [[5.0, 7.0], [3.0, 9.0]]
    r3 = rank_ref.rank(tab, 3)
    assert r3["typ_idx"][1].tolist() == [2, 0, -1] and np.isnan(r3["typ_score"][1, 2]) and r3["fringe_idx"][0].tolist() == [1, 5, 6]
    halves = [rank_ref.rank(tab[:, :3], 3), rank_ref.rank(tab[:, 3:], 3, index_base=3)]
    whole = rank_ref.merge(halves, 3)
    for k, v in r3.items():
        assert np.array_equal(whole[k], v, equal_nan=True), k
    assert rank_ref.rank(tab, 2, n_valid=5)["count"].tolist() == [1, 2]


# ---------------------------------------------------------------------------------------------- Predictor.exemplars over a stand-in
class TableWorker(FakeWorker):
    """The oracle-backed stand-in with the calls `Predictor.exemplars` makes: a numpy table a_k(i) = log w_k - |x_i - c_k|^2 in Float32,
    c_k the predictive means, ranked piece by piece with tests/tools/rank_ref.py."""
    made = []

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.uploads, self.accumulated, self.closed = [], [], False
        TableWorker.made.append(self)

    def close(self):
        self.closed = True

    def upload_points(self, X):
        X = np.asarray(X)
        assert X.shape == (self.n, self.D) and X.dtype == np.float32, (X.shape, X.dtype)      # never a short upload
        super().upload_points(X)
        self.uploads.append(X.shape[0])

    def set_predictive_niw(self, m, R, logdet, df, weights):
        self.centres, self.logw, self.K = np.asarray(m, np.float32), np.log(np.asarray(weights, np.float32)), len(weights)

    def table(self):
        d = ((self.X[None, :, :] - self.centres[:, None, :]) ** 2).sum(-1, dtype=np.float32)
        return (self.logw[:, None] - d).astype(np.float32)                                    # (K, n)

    def rank_begin(self, m, which):
        self.m, self.which, self.pieces = int(m), int(which), []

    def rank_accumulate(self, index_base, n_valid):
        assert 0 <= n_valid <= self.n
        self.accumulated.append((int(index_base), int(n_valid)))
        self.pieces.append(rank_ref.rank(self.table(), self.m, index_base=index_base, n_valid=n_valid))

    def rank_read(self, device=None):
        assert device is None
        r = rank_ref.merge(self.pieces, self.m) if self.pieces else rank_ref.rank(np.zeros((self.K, 0), np.float32), self.m)
        r["skipped"] = np.array([r["skipped"]], np.int64)
        return r


def model(D, K, seed=0):
    """What a Predictor reads of a fitted NIW model; cluster 0 has its mean exactly at the origin, where the padding of a short slab sits."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((3 * K, D, D)) * 0.1 + np.eye(D)
    m = rng.standard_normal((3 * K, D))
    m[0] = 0.0
    post = dict(kappa=1 + rng.random(3 * K), nu=D + 3 + rng.random(3 * K), m=m, U=np.triu(A) + 2 * np.eye(D), logdet_psi=np.zeros(3 * K))
    s = types.SimpleNamespace(K=K, prior=types.SimpleNamespace(kind=0, dim=D), post=post, alpha=10.0, points_count=rng.integers(5, 50, K),
                              wk=types.SimpleNamespace(device=0))
    return types.SimpleNamespace(sampler=s)


N = 3 * 256 + 5


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("cap", [N, 1, 256, 100])      # capacity = n | a divisor of n (773 is prime: 1) | two that leave a short slab
@pytest.mark.parametrize("m", [1, 16])
def test_exemplars_equal_the_definitions_for_every_capacity(score, cap, m):
    D, K = 3, 4
    rng = np.random.default_rng(5)
    X = rng.standard_normal((D, N)).astype(np.float32)
    X[:, 7] = X[:, 400] = X[:, 600]                                   # the same point at three indices: ties across slabs
    p = score.Predictor(model(D, K), capacity=cap, worker_factory=TableWorker)
    wk = p._wk
    whole = TableWorker(0, D, N)
    whole.centres, whole.logw, whole.K = wk.centres, wk.logw, wk.K
    whole.upload_points(np.ascontiguousarray(X.T))
    want = rank_ref.rank(whole.table(), m)
    assert want["count"].min() > 0 and want["count"].sum() == N
    got = p.exemplars(X, m)
    assert isinstance(got, score.Exemplars) and isinstance(got.skipped, int)
    assert wk.uploads == [cap] * -(-N // cap)
    assert wk.accumulated == [(lo, min(cap, N - lo)) for lo in range(0, N, cap)]
    assert same(got.typical_idx, want["typ_idx"]) and same(got.typical_score, want["typ_score"])
    assert same(got.fringe_idx, want["fringe_idx"]) and same(got.fringe_score, want["fringe_score"])
    assert same(got.count, want["count"]) and got.skipped == want["skipped"] == 0
    assert got.typical_idx.max() < N and got.count.sum() + got.skipped == N       # the padding took no part
    only = p.exemplars(X, m, which="fringe")
    assert only.typical_idx is None and only.typical_score is None and same(only.fringe_idx, want["fringe_idx"]) and wk.which == 2
    assert p.exemplars(X, m, which="typical").fringe_idx is None and wk.which == 1
    p.close()


def test_one_shot_and_empty_data(score):
    D, K = 3, 4
    X = np.random.default_rng(6).standard_normal((D, 50)).astype(np.float32)
    mdl = model(D, K)
    before = len(TableWorker.made)
    a = score.exemplars(mdl, X, 4, capacity=16, worker_factory=TableWorker, which="typical")
    assert len(TableWorker.made) == before + 1 and TableWorker.made[-1].closed
    with score.Predictor(mdl, capacity=64, worker_factory=TableWorker) as p:
        b = p.exemplars(X, 4)
        e = p.exemplars(X[:, :0], 4)
    assert same(a.typical_idx, b.typical_idx) and a.fringe_idx is None
    assert np.all(e.typical_idx == -1) and np.isnan(e.fringe_score).all() and e.count.tolist() == [0] * K and e.skipped == 0
    host = importlib.import_module(score.__name__.rsplit(".", 1)[0])
    assert host.exemplars is score.exemplars and host.Exemplars is score.Exemplars


def test_refusals(score, monkeypatch):
    p = score.Predictor(model(3, 4), capacity=10, worker_factory=TableWorker)
    X = np.zeros((3, 5), np.float32)
    for m in (0, -1, 65):
        with pytest.raises(ValueError, match="m must"):
            p.exemplars(X, m)
    with pytest.raises(ValueError, match="which"):
        p.exemplars(X, 2, which="edge")
    with pytest.raises(ValueError, match="dimension"):
        p.exemplars(np.zeros((4, 5)), 2)
    fake = types.SimpleNamespace(device_index=1, torch_device="cuda:1", shape=(3, 5))      # a tensor on another device than the Predictor's
    monkeypatch.setattr(score._tensors, "as_device_points", lambda data: fake)
    with pytest.raises(ValueError, match="device"):
        p.exemplars(object(), 2)
    monkeypatch.undo()
    p.close()
    with pytest.raises(RuntimeError, match="closed"):
        p.exemplars(X, 2)
