"""CPU-side checks of the cluster overlap (include/dpmm_hip_overlap.h) and of the merge hierarchy (host/hierarchy.py): the header
compiles as C, its functions are bound, exported and built from csrc/overlap.hip; the definitions (tests/tools/overlap_ref.py) on a
table written by hand; `Predictor.overlap` walks the slabs over a stand-in worker that keeps a numpy table and equals the definitions
whatever the capacity; `merge_tree` on a matrix written by hand, its closure under merging on random probabilities, relabelling and the
refusals."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package
from tools import overlap_ref
import test_rank_cpu as R

HEADER = os.path.join(ROOT, "include", "dpmm_hip_overlap.h")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


@pytest.fixture(scope="module")
def hier(pkg):
    return importlib.import_module(pkg.__name__ + ".host.hierarchy")


# ---------------------------------------------------------------------------------------------- the C boundary
def test_header_compiles_as_c_and_is_bound_exported_and_built(pkg):
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER])
    hdr = open(HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", body)))
    assert declared == ["dpmm_overlap_accumulate", "dpmm_overlap_begin", "dpmm_overlap_read"]
    binding = importlib.import_module(pkg.__name__ + ".binding")
    assert sorted(n for n, _, _ in binding.ABI_OVERLAP) == declared
    others = (binding.ABI + binding.ABI_TENSOR + binding.ABI_SCORE + binding.ABI_RANK + binding.ABI_TRACE + binding.ABI_MISSING + binding.ABI_CSC
              + binding.ABI_SAMPLE + binding.ABI_PROJECT)
    assert not set(declared) & set(n for n, _, _ in others)
    for name in ("overlap_begin", "overlap_accumulate", "overlap_read"):
        assert callable(getattr(binding.Worker, name)), name
    assert int(re.search(r"#define DPMM_OVERLAP_PARTIAL_BLOCKS (\d+)", hdr).group(1)) == binding.OVERLAP_PARTIAL_BLOCKS
    struct = body[body.index("typedef struct {"):body.index("} dpmm_overlap_out;")]
    assert re.findall(r"\*\s*([a-z_]+);", struct) == [f[0] for f in binding.OverlapOut._fields_]
    assert re.findall(r"(double|int64_t)\s*\*", struct) == ["double", "double", "int64_t", "int64_t"]
    mk = open(os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "build/overlap.o" in objs
    api = re.search(r"^build/dpmm_api\.o:(.*)$", mk, flags=re.M).group(1).split()
    assert "../../include/dpmm_hip_overlap.h" in api
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for n in declared:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                               # additive: the version stays
    host = importlib.import_module(pkg.__name__ + ".host")
    assert callable(host.overlap) and callable(host.Predictor.overlap) and callable(host.merge_tree)
    assert host.Overlap._fields == ("matrix", "mass", "count", "skipped") and host.MergeTree._fields[:3] == ("merges", "similarity", "Z")


# ---------------------------------------------------------------------------------------------- the reference itself
def test_overlap_ref_on_a_table_written_by_hand():
    nan, inf = np.nan, np.inf
    l2, l3 = np.float32(np.log(2.0)), np.float32(np.log(3.0))
    #                 0    1    2    3     4     5    6    7
    tab = np.array([[0.0, 5.0, l3,  nan, -inf, 0.0, 0.0, 0.5],
                    [0.0, 5.0, 0.0, 8.0, -inf, l2, -inf, inf]], np.float32)
    # point 0, 1: a tie (1/2, 1/2; the label is the first maximum); 2: (3/4, 1/4); 3: a NaN; 4: a row of -Inf; 5: (1/3, 2/3); 6: (1, 0);
    # 7: a +Inf entry
    P, lab, part = overlap_ref.probs(tab)
    assert list(lab) == [1, 1, 1, 1, 1, 2, 1, 2]
    assert list(part) == [True, True, True, False, False, True, True, False]
    want = np.zeros((8, 2))
    want[[0, 1]] = 0.5
    want[2], want[5], want[6] = (0.75, 0.25), (1 / 3, 2 / 3), (1.0, 0.0)
    assert np.abs(P - want).max() <= 2.0 ** -22 and np.all(P[~part] == 0) and P.dtype == np.float32
    r = overlap_ref.overlap(tab)
    assert r["skipped"] == 3 and r["count"].tolist() == [4, 1] and r["count"].dtype == np.int64
    Q = P.astype(np.float64)
    exact = np.array([[sum(float(a) * float(a) for a in Q[:, 0]), sum(float(a) * float(b) for a, b in Q)],
                      [0.0, sum(float(b) * float(b) for b in Q[:, 1])]])
    exact[1, 0] = exact[0, 1]
    assert overlap_ref.close(r["overlap"], exact, 8) and overlap_ref.close(r["mass"], Q.sum(0), 8)
    assert np.array_equal(r["overlap"], r["overlap"].T)
    assert abs(r["overlap"][0, 0] - (0.25 + 0.25 + 0.5625 + 1 / 9 + 1)) < 1e-6 and abs(r["mass"].sum() - 5) < 1e-6
    # n_valid cuts the table: points 0..2 only, nothing skipped
    cut = overlap_ref.overlap(tab, n_valid=3)
    assert cut["skipped"] == 0 and cut["count"].tolist() == [3, 0] and overlap_ref.close(cut["overlap"], Q[:3].T @ Q[:3], 3)
    halves = overlap_ref.add([overlap_ref.overlap(tab[:, :3]), overlap_ref.overlap(tab[:, 3:])])
    assert overlap_ref.close(halves["overlap"], r["overlap"], 8) and halves["count"].tolist() == [4, 1] and halves["skipped"] == 3
    assert overlap_ref.bound(8) == 8 * 2.0 ** -52


# ---------------------------------------------------------------------------------------------- Predictor.overlap over a stand-in
class OverlapWorker(R.TableWorker):
    """tests/test_rank_cpu.py's table-keeping stand-in with the calls `Predictor.overlap` makes, piece by piece through overlap_ref."""

    def overlap_begin(self):
        self.ov_pieces, self.ov_calls = [], []

    def overlap_accumulate(self, n_valid):
        assert 0 <= n_valid <= self.n
        self.ov_calls.append(int(n_valid))
        self.ov_pieces.append(overlap_ref.overlap(self.table(), n_valid=n_valid))

    def overlap_read(self):
        r = overlap_ref.add(self.ov_pieces) if self.ov_pieces else overlap_ref.overlap(np.zeros((self.K, 0), np.float32))
        r["skipped"] = np.array([r["skipped"]], np.int64)
        return r


N = 29


@pytest.mark.parametrize("cap", [1, 7, N, N + 5])
def test_predictor_overlap_equals_the_definitions_for_every_capacity(score, cap):
    D, K = 3, 4
    rng = np.random.default_rng(5)
    X = rng.standard_normal((D, N)).astype(np.float32)
    p = score.Predictor(R.model(D, K), capacity=cap, worker_factory=OverlapWorker)
    wk = p._wk
    whole = OverlapWorker(0, D, N)
    whole.centres, whole.logw, whole.K = wk.centres, wk.logw, wk.K
    whole.upload_points(np.ascontiguousarray(X.T))
    want = overlap_ref.overlap(whole.table())
    got = p.overlap(X)
    assert isinstance(got, score.Overlap) and isinstance(got.skipped, int) and got.skipped == 0
    assert all(isinstance(a, np.ndarray) for a in got[:3]) and got.matrix.dtype == np.float64 and got.count.dtype == np.int64
    assert wk.uploads == [cap] * -(-N // cap)                                     # never a short upload ...
    assert wk.ov_calls == [min(cap, N - lo) for lo in range(0, N, cap)]         # ... the padding is cut by n_valid
    assert overlap_ref.close(got.matrix, want["overlap"], N) and overlap_ref.close(got.mass, want["mass"], N)
    assert np.array_equal(got.count, want["count"]) and got.count.sum() == N     # the padded points of the short slab took no part
    assert abs(got.mass.sum() - N) <= N * K * 2.0 ** -24
    e = p.overlap(X[:, :0])
    assert e.matrix.shape == (K, K) and not e.matrix.any() and not e.mass.any() and e.count.tolist() == [0] * K and e.skipped == 0
    p.close()
    with pytest.raises(RuntimeError, match="closed"):
        p.overlap(X)


def test_one_shot_and_a_worker_that_cannot(score):
    D, K = 3, 4
    X = np.random.default_rng(6).standard_normal((D, 50)).astype(np.float32)
    mdl = R.model(D, K)
    before = len(R.TableWorker.made)
    a = score.overlap(mdl, X, capacity=16, worker_factory=OverlapWorker)
    assert len(R.TableWorker.made) == before + 1 and R.TableWorker.made[-1].closed
    with score.Predictor(mdl, capacity=64, worker_factory=OverlapWorker) as p:
        b = p.overlap(X)
        with pytest.raises(ValueError, match="dimension"):
            p.overlap(np.zeros((4, 5), np.float32))
    assert overlap_ref.close(a.matrix, b.matrix, 50) and np.array_equal(a.count, b.count)
    host = importlib.import_module(score.__name__.rsplit(".", 1)[0])
    assert host.overlap is score.overlap and host.Overlap is score.Overlap
    with score.Predictor(mdl, capacity=64, worker_factory=R.TableWorker) as p:       # a worker without overlap_begin
        with pytest.raises(RuntimeError, match="overlap"):
            p.overlap(X)


# ---------------------------------------------------------------------------------------------- merge_tree
def hand_matrix():
    # clusters 1 and 2 overlap strongly, 3 and 4 exactly as strongly (a tie), the two pairs weakly; diagonals 4 so that s = O / 4
    return np.array([[4.0, 2.0, 0.4, 0.0],
                     [2.0, 4.0, 0.0, 0.4],
                     [0.4, 0.0, 4.0, 2.0],
                     [0.0, 0.4, 2.0, 4.0]])


def test_merge_tree_on_a_matrix_written_by_hand(hier, score):
    O = hand_matrix()
    ov = score.Overlap(O, np.array([5.0, 6.0, 7.0, 8.0]), np.array([1, 2, 3, 4], np.int64), 9)
    t = hier.merge_tree(ov)
    assert isinstance(t, hier.MergeTree) and t.merges.dtype == np.int64 and t.merges.shape == (3, 2) and t.similarity.shape == (3,)
    # the tie s(1, 2) = s(3, 4) = 0.5 goes to (1, 2); then (3, 4); then the two groups: (0.4 + 0.4) / sqrt(12 * 12)
    assert t.merges.tolist() == [[1, 2], [3, 4], [1, 3]]
    assert np.allclose(t.similarity, [0.5, 0.5, 0.8 / 12], rtol=1e-15)
    assert t.Z.shape == (3, 4) and t.Z[:, :2].tolist() == [[0, 1], [2, 3], [4, 5]] and t.Z[:, 3].tolist() == [2, 2, 4]
    assert np.allclose(t.Z[:, 2], 1 - t.similarity)
    assert t.cut(groups=4).tolist() == [1, 2, 3, 4] and t.cut(groups=3).tolist() == [1, 1, 2, 3]
    assert t.cut(groups=2).tolist() == [1, 1, 2, 2] and t.cut(groups=1).tolist() == [1, 1, 1, 1]
    assert t.cut(groups=2).dtype == np.int64
    assert t.cut(similarity=0.6).tolist() == [1, 2, 3, 4]                       # the first merge is already below 0.6
    assert t.cut(similarity=0.5).tolist() == [1, 1, 2, 2] and t.cut(similarity=0.0).tolist() == [1, 1, 1, 1]
    c = t.overlap(groups=2)
    assert c.matrix.tolist() == [[12.0, 0.8], [0.8, 12.0]] and c.mass.tolist() == [11.0, 15.0] and c.count.tolist() == [3, 7] and c.skipped == 9
    assert t.overlap(groups=4).matrix.tolist() == O.tolist()
    # the group numbering follows the smallest member: 2 and 4 merge first, the group {2, 4} is numbered after {1}
    P = O[np.ix_([0, 2, 1, 3], [0, 2, 1, 3])]                                   # now (1, 3) and (2, 4) are the strong pairs
    P[1, 3] = P[3, 1] = 3.0
    t2 = hier.merge_tree(P)
    assert t2.merges.tolist() == [[2, 4], [1, 3], [1, 2]] and t2.cut(groups=3).tolist() == [1, 2, 3, 2]
    assert np.allclose(t2.overlap(groups=3).mass, [P[0].sum(), P[1].sum() + P[3].sum(), P[2].sum()])      # a bare matrix: masses are row sums
    assert t2.overlap(groups=3).count.tolist() == [0, 0, 0]


def test_a_cluster_with_zero_mass_merges_last(hier):
    O = hand_matrix()
    O[1, :] = 0.0
    O[:, 1] = 0.0                                                               # cluster 2 is empty: s = 0 with everyone
    t = hier.merge_tree(O)
    assert t.merges.tolist() == [[3, 4], [1, 3], [1, 2]] and t.similarity[2] == 0.0 and t.Z[2, 2] == 1.0
    one = hier.merge_tree(np.array([[2.5]]))
    assert one.merges.shape == (0, 2) and one.cut(groups=1).tolist() == [1] and one.overlap(groups=1).matrix.tolist() == [[2.5]]


def test_the_hierarchy_is_closed_under_merging(hier, score):
    n, K = 500, 7
    rng = np.random.default_rng(11)
    A = rng.standard_normal((n, K)) * 3
    P = np.exp(A - A.max(1, keepdims=True))
    P = (P / P.sum(1, keepdims=True)).astype(np.float32).astype(np.float64)
    lab = P.argmax(1) + 1
    ov = score.Overlap(P.T @ P, P.sum(0), np.bincount(lab - 1, minlength=K).astype(np.int64), 0)
    t = hier.merge_tree(ov)
    tol = (n + K) * 2.0 ** -52                                                  # the sums over n, and at most K more roundings of the merges
    for g in range(1, K + 1):
        groups = t.cut(groups=g)
        assert sorted(set(groups.tolist())) == list(range(1, g + 1))
        first = [int(np.flatnonzero(groups == j)[0]) for j in range(1, g + 1)]
        assert first == sorted(first)                                           # numbered by smallest member
        Q = np.stack([P[:, groups == j].sum(1) for j in range(1, g + 1)], axis=1)
        c = t.overlap(groups=g)
        want = Q.T @ Q
        assert np.all(np.abs(c.matrix - want) <= tol * want), g
        assert np.array_equal(c.matrix, c.matrix.T)
        assert np.all(np.abs(c.mass - Q.sum(0)) <= tol * Q.sum(0))
        assert np.array_equal(c.count, np.bincount(groups[lab - 1] - 1, minlength=g))
        assert np.array_equal(t.relabel(lab, groups=g), groups[lab - 1])
    for j, s in enumerate(t.similarity):
        below = np.flatnonzero(t.similarity < s)
        steps = int(below[0]) if below.size else K - 1
        assert np.array_equal(t.cut(similarity=s), t.cut(groups=K - steps)), j


def test_relabel_and_refusals(hier):
    import torch
    t = hier.merge_tree(hand_matrix())
    lab = np.array([[1, 2, 3], [4, 4, 1]])
    assert t.relabel(lab, groups=2).tolist() == [[1, 1, 2], [2, 2, 1]] and t.relabel(lab, groups=2).dtype == np.int64
    tl = torch.tensor([4, 1, 3, 2], dtype=torch.int32)
    out = t.relabel(tl, similarity=0.5)
    assert torch.is_tensor(out) and out.dtype == torch.int64 and out.device == tl.device and out.tolist() == [2, 1, 2, 1]
    for kw in ({}, dict(groups=2, similarity=0.5), dict(groups=0), dict(groups=5), dict(groups=2.5), dict(similarity=float("nan"))):
        with pytest.raises(ValueError):
            t.cut(**kw)
        with pytest.raises(ValueError):
            t.overlap(**kw)
    with pytest.raises(ValueError, match="labels"):
        t.relabel(np.array([0, 1]), groups=2)
    with pytest.raises(ValueError, match="labels"):
        t.relabel(torch.tensor([1, 5]), groups=2)
    with pytest.raises(ValueError, match="integers"):
        t.relabel(np.array([1.0]), groups=2)
    for bad in (np.zeros((2, 3)), np.zeros(4), np.array([[1.0, -1.0], [-1.0, 1.0]]), np.array([[np.nan]])):
        with pytest.raises(ValueError):
            hier.merge_tree(bad)
