"""CPU-side checks of the explanations by groups of features (include/dpmm_hip_explain_groups.h): the header compiles as C, its functions
are bound, exported and built from csrc/explain_group.hip; the Float64 reference of tests/tools/explain_groups_ref.py against a direct
conditional, against the per-feature and the whole-point references, and its calibration on Student-t draws; the bound tells a wrong
grouping from the right one on every case of the GPU tests; `group_factors`, the argument checks of `Predictor.explain_groups` and the
lazy re-forming of its tables over a stand-in worker."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package
from tools import explain_groups_ref as EG
from tools import explain_ref as E
from tools import sample_ref as SR
from tools import typicality_ref as T

HEADER = os.path.join(ROOT, "include", "dpmm_hip_explain_groups.h")
FUNCS = ["dpmm_explain_groups_points", "dpmm_explain_groups_points_device", "dpmm_set_explain_groups"]
CSRC = os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


@pytest.fixture(scope="module")
def host(pkg):
    return importlib.import_module(pkg.__name__ + ".host")


@pytest.fixture(scope="module")
def condition(pkg):
    return importlib.import_module(pkg.__name__ + ".host.condition")


# ---------------------------------------------------------------------------------------------- the C boundary
def test_header_compiles_as_c_and_is_bound_exported_and_built(pkg, host):
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER])
    hdr = open(HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", body))) == FUNCS
    binding = importlib.import_module(pkg.__name__ + ".binding")
    assert sorted(n for n, _, _ in binding.ABI_EXPLAIN_GROUPS) == FUNCS
    others = (binding.ABI + binding.ABI_TENSOR + binding.ABI_SCORE + binding.ABI_RANK + binding.ABI_OVERLAP + binding.ABI_BATCHSTATS + binding.ABI_COUNTSTATS
              + binding.ABI_TYPICALITY + binding.ABI_EXPLAIN + binding.ABI_HOLDOUT + binding.ABI_TRACE + binding.ABI_MISSING + binding.ABI_IMPUTE + binding.ABI_CSC
              + binding.ABI_SAMPLE + binding.ABI_PROJECT + binding.ABI_REGRESS + binding.ABI_RECOMMEND)
    assert not set(FUNCS) & set(n for n, _, _ in others)
    for name in ("set_explain_groups", "explain_groups_points_raw", "explain_groups_points_into"):
        assert callable(getattr(binding.Worker, name)), name
    struct = body[body.index("typedef struct {"):body.index("} dpmm_explain_groups_out;")]
    fields = re.findall(r"(float|int64_t|int32_t)\s*(\*?)\s*([A-Za-z_]+);", struct)
    assert [f[2] for f in fields] == [f[0] for f in binding.ExplainGroupsOut._fields_]
    ctype = {("int32_t", ""): ctypes.c_int32, ("int64_t", ""): ctypes.c_int64}
    assert [ctype.get((t, p), ctypes.c_void_p) for t, p, _ in fields] == [f[1] for f in binding.ExplainGroupsOut._fields_]
    assert [f[0] for f in binding.ExplainGroupsOut._fields_[:5]] == [f[0] for f in binding.TypicalityOut._fields_]      # the five fields of dpmm_typicality_out first
    assert int(re.search(r"#define DPMM_EXPLAIN_MAX_GROUPS (\d+)", hdr).group(1)) == binding.EXPLAIN_MAX_GROUPS == 64
    assert f"EXPLAIN_MAX_GROUPS = {binding.EXPLAIN_MAX_GROUPS};" in open(os.path.join(CSRC, "dpmm_kernels.h")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "build/explain_group.o" in re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "../../include/dpmm_hip_explain_groups.h" in re.search(r"^build/dpmm_api\.o:(.*)$", mk, flags=re.M).group(1).split()
    assert "-ffp-contract=off" in re.search(r"^FLAGS\s*=(.*)$", mk, flags=re.M).group(1).split()            # the flags of explain.o: one pattern rule
    hip = open(os.path.join(CSRC, "explain_group.hip")).read()
    assert "miss_rz<NT>" in hip and "miss_rty<NT>" in hip and '#include "missing_device.h"' in hip
    assert "atomicAdd" not in hip and "__syncthreads" not in hip                        # every output word has one writer; the waves share nothing
    jl = open(os.path.join(ROOT, "julia", "gpu_explain_groups.jl")).read()
    assert set(re.findall(r":(dpmm_[a-z0-9_]+)", jl)) == {"dpmm_set_explain_groups", "dpmm_explain_groups_points"}
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for n in FUNCS:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                               # additive: the version stays
    assert callable(host.explain_groups) and callable(host.Predictor.explain_groups)
    assert host.GroupExplanation._fields == ("labels", "mahalanobis", "tail", "group_mahalanobis", "group_tail", "names", "sizes", "skipped", "incomplete")


# ---------------------------------------------------------------------------------------------- the reference itself
def one_cluster(D, df, seed):
    post, m, A, dfs = SR.niw_model(D, 1, df, seed)
    R = np.linalg.inv(A)                                             # Sigma^-1 = R'R, Sigma = A A'
    return post, m, A, dfs, T.worker_params(m, R, dfs)


def sized_groups(D):
    """Groups of sizes 1, 2, D - 1 and D (each a case of its own where they cannot be disjoint), spread over the features."""
    out = [[[D - 1]], [list(range(D))]]
    if D >= 2:
        out.append([[0, D - 1]])
        out.append([[d for d in range(D) if d != D // 2]])
    if D >= 4:
        out.append([[1], [0, D - 1]])                                # two groups in one call
    return out


@pytest.mark.parametrize("D", [2, 5, 64])
def test_reference_equals_a_direct_conditional(D):
    """Sigma = (R'R)^-1, block G conditioned on the rest with numpy.linalg.solve, its squared distance under the conditional scale: q_G and
    f_G of the reference to 1e-9 relative."""
    rng = np.random.default_rng(D)
    for df in (4.0, 1e5):
        _, m, A, dfs, (m32, R32, df32) = one_cluster(D, df, 30 + D)
        x = (m[0] + (A[0] @ rng.standard_normal((D, 6))).T * np.array([0.3, 1, 1, 2, 5, 20])[:, None]).astype(np.float32)
        for groups in sized_groups(D):
            ref = EG.reference(x.T, np.zeros(6, np.int64), m32, R32, df32, groups)
            for i in range(6):
                for j, g in enumerate(groups):
                    qG, fG = EG.direct_conditional(x[i], m32[0], R32[0], df32[0], g)
                    assert abs(ref.qg[i, j] - qG) <= 1e-9 * qG and abs(ref.f[i, j] - fG) <= 1e-9 * fG, (D, df, groups, i)
            assert np.all(ref.q[:, None] - ref.qg >= -1e-9 * ref.q[:, None])                              # q_-G >= 0


@pytest.mark.parametrize("D", [2, 5, 64])
def test_reference_identities_one_feature_and_all_features(D):
    rng = np.random.default_rng(100 + D)
    for df in (4.0, 1e5):
        _, m, A, dfs, (m32, R32, df32) = one_cluster(D, df, 40 + D)
        x = (m[0] + (A[0] @ rng.standard_normal((D, 8))).T * np.array([0.3, 1, 1, 1, 2, 5, 20, 0.1])[:, None]).astype(np.float32)
        lab0 = np.zeros(8, np.int64)
        one = EG.reference(x.T, lab0, m32, R32, df32, [[d] for d in range(D)][:64])
        feat = E.reference(x.T, lab0, m32, R32, df32)
        assert np.allclose(one.f, feat.t[:, :64] ** 2, rtol=1e-9, atol=0) and np.allclose(one.tail, feat.tail[:, :64], rtol=1e-9, atol=1e-300)
        full = EG.reference(x.T, lab0, m32, R32, df32, [list(range(D))])
        q, _, tail = T.reference(x.T, lab0, m32, R32, df32)
        assert np.allclose(full.qg[:, 0], q, rtol=1e-9, atol=0) and np.allclose(full.f[:, 0], q, rtol=1e-9, atol=0)
        assert np.allclose(full.tail[:, 0], tail, rtol=1e-9, atol=1e-300)


# seeds fixed here, on the CPU: each KS distance is printed and lies under 0.0115, the 1 % critical distance 1.63 / sqrt(n) at n = 20000
KS_CASES = [(8, 4.0, 41), (64, 1e5, 42)]


@pytest.mark.parametrize("D,df,seed", KS_CASES)
def test_reference_group_tails_of_student_t_draws_are_uniform(D, df, seed):
    n = 20000
    _, m, A, dfs, (m32, R32, df32) = one_cluster(D, df, 700 + seed)
    x = SR.niw_points(m, A, dfs, np.zeros(n, np.int64), np.arange(n), seed)
    groups = [[1], [0, 2, D - 1], list(range(3, 3 + D // 2))]                                             # sizes 1, 3 and D / 2, disjoint
    ref = EG.reference(x.T.astype(np.float32), np.zeros(n, np.int64), m32, R32, df32, groups)
    for j, g in enumerate(groups):
        dist = T.ks_uniform(ref.tail[:, j])
        print(f"D = {D} df = {df:g} group of {len(g)}: KS distance {dist:.5f}, bound 0.0115")
        assert dist < 0.0115
        assert T.ks_uniform(np.clip(ref.tail[:, j] * 1.05, 0, 1)) > 0.0115                                # the test has power: a 5 % miscalibration is seen


# ---------------------------------------------------------------------------------------------- the bound discriminates
@pytest.mark.parametrize("heavy", [True, False], ids=["df=D+3", "df=1e5"])
@pytest.mark.parametrize("case", EG.CASES, ids=EG.CASE_IDS)
def test_bound_tells_a_wrong_grouping_from_the_right_one(case, heavy):
    """Every case of tests/test_gpu_explain_groups.py: the reference of the grouping with one feature exchanged between the first two
    groups lies outside twice the bound on at least one point.  (A case of one group has nothing to exchange.)"""
    D, name, groups = case
    wrong_groups = EG.swapped(groups)
    if wrong_groups is None:
        assert len(groups) == 1 and groups[0] == list(range(D))
        return
    post, m, A, df = EG.case_model(D, heavy)
    X, lab0 = EG.case_points_cpu(D, heavy, groups)
    params = T.worker_params(m, np.linalg.inv(A), df)
    ref = EG.reference(X, lab0, *params, groups)
    wrong = EG.reference(X, lab0, *params, wrong_groups)
    rel = np.max(ref.qg_bound / np.maximum(ref.qg, 1e-300))
    print(name, "D", D, "largest twice-bound relative to q_G:", 2 * rel, "points and groups told apart:", int((np.abs(ref.qg - wrong.qg) > 2 * ref.qg_bound + 2 * wrong.qg_bound).sum()))
    assert EG.discriminates(ref, wrong)


# ---------------------------------------------------------------------------------------------- group_factors
@pytest.mark.parametrize("D", [5, 64, 130])
def test_group_factors_invert_the_blocks(condition, D):
    K = 3
    _, m, A, dfs = SR.niw_model(D, K, 9.0, 5 + D)
    R = np.linalg.inv(A).astype(np.float32)
    groups = [[0], [1, D - 1], list(range(2, D - 1))]
    Ws = condition.group_factors(R, groups, packed=False)
    A64 = np.einsum("kji,kjl->kil", np.triu(R.astype(np.float64)), np.triu(R.astype(np.float64)))
    packed = condition.group_factors(R.reshape(K, D * D), groups)
    assert packed.dtype == np.float64 and packed.shape == (K, sum(len(g) * (len(g) + 1) // 2 for g in groups))
    at = 0
    for g, W in zip(groups, Ws):
        s = len(g)
        assert W.shape == (K, s, s) and np.all(np.triu(W, 1) == 0)
        for k in range(K):
            AGG = A64[k][np.ix_(g, g)]
            assert np.abs(W[k] @ AGG @ W[k].T - np.eye(s)).max() <= 1e-10, (D, s, k)
            assert np.array_equal(packed[k, at:at + s * (s + 1) // 2], W[k][np.tril_indices(s)])          # rows of the lower triangle, one after the other
        at += s * (s + 1) // 2


# ---------------------------------------------------------------------------------------------- argument checks and lazy tables over a stand-in
def stand_in():
    from fake_worker import FakeWorker

    class Quiet(FakeWorker):
        """Takes the predictive parameters, counts the table uploads and fills nothing."""
        asked = 0
        tables = []

        def set_predictive_niw(self, *a):
            pass

        def set_predictive_mult(self, *a):
            pass

        def set_explain_groups(self, groups, W):
            Quiet.tables.append(([list(g) for g in groups], np.array(W)))

        def explain_groups_points_into(self, views):
            Quiet.asked += 1
            for v in views.values():
                v[...] = 0
            return 0, 0

        def upload_points(self, *a, **kw):
            pass
    Quiet.asked, Quiet.tables = 0, []
    return Quiet


def niw_predictor(score, D, K, factory):
    post, _, _, _ = SR.niw_model(D, K, 9.0, 3)
    p = score.Predictor.__new__(score.Predictor)
    p._setup(0, D, 10.0, np.full(K, 50.0), post, 16, 0, factory)
    return p


def test_refusals(score):
    Quiet = stand_in()
    D, K = 6, 2
    X = np.zeros((D, 5), np.float32)
    mult = score.Predictor.__new__(score.Predictor)
    mult._setup(1, D, 10.0, np.full(K, 5.0), dict(alpha=np.ones((K, D), np.float32)), 16, 0, Quiet)
    with pytest.raises(ValueError, match="Multinomial.*closed-form tail"):
        mult.explain_groups(X, [[0]])
    mult.close()
    p = niw_predictor(score, D, K, Quiet)
    for bad, why in (([], "between 1 and 64"), ([[0], []], "empty"), ([[0, 0]], "repeats"), ([[0, 1], [1, 2]], "overlaps"), ([[0, D]], "0..5"), ([[-1]], "0..5"),
                     ([[0.5]], "integer"), (3, "sequence"), ([[d] for d in range(65)], "between 1 and 64"), ({"a": [0], "b": [0]}, "'b' overlaps")):
        with pytest.raises(ValueError, match=why):
            p.explain_groups(X, bad)
    assert Quiet.asked == 0 and Quiet.tables == []
    wide = niw_predictor(score, 70, K, Quiet)
    with pytest.raises(ValueError, match="between 1 and 64"):
        wide.explain_groups(np.zeros((70, 5), np.float32), [[d] for d in range(65)])
    wide.close()
    p.close()
    with pytest.raises(RuntimeError, match="closed"):
        p.explain_groups(X, [[0]])
    from fake_worker import FakeWorker
    q = niw_predictor(score, D, K, type("Bare", (FakeWorker,), {"set_predictive_niw": lambda self, *a: None}))
    with pytest.raises(RuntimeError, match="explain groups"):        # a worker without dpmm_explain_groups_points
        q.explain_groups(X, [[0]])
    q.close()
    assert Quiet.asked == 0 and Quiet.tables == []


def test_tables_are_formed_once_per_groups_and_model(score, condition):
    Quiet = stand_in()
    D, K = 6, 2
    X = np.zeros((D, 40), np.float32)                                # three slabs of 16
    p = niw_predictor(score, D, K, Quiet)
    got = p.explain_groups(X, {"b": [4, 2], "a": [0]})               # sorted on the way in, the order of the groups kept
    assert got.names == ("b", "a") and got.sizes == (2, 1) and got.group_tail.shape == (2, 40) and got.group_mahalanobis.shape == (2, 40)
    assert got.group_tail.T.flags.c_contiguous                       # a .T view of point-major memory
    assert len(Quiet.tables) == 1 and Quiet.tables[0][0] == [[2, 4], [0]] and Quiet.asked == 3
    R = np.asarray(p._predictive_args()[1][1], np.float32)
    assert np.array_equal(Quiet.tables[0][1], condition.group_factors(R, [[2, 4], [0]]))
    assert p.explain_groups(X, [[2, 4], [0]]).names is None
    p.explain_groups(X, [(4, 2), (0,)])
    assert len(Quiet.tables) == 1                                    # the same groups: no new upload
    p.explain_groups(X, [[0], [2, 4]])
    assert len(Quiet.tables) == 2 and Quiet.tables[1][0] == [[0], [2, 4]]      # other groups (another order is another table)
    p._reload()                                                      # what absorb and grow do with the new posterior
    p.explain_groups(X, [[0], [2, 4]])
    p.explain_groups(X, [[0], [2, 4]])
    assert len(Quiet.tables) == 3
    p.close()
