"""CPU-side checks of the per-feature explanations (include/dpmm_hip_explain.h): the header compiles as C, its functions are bound, exported
and built from csrc/explain.hip; the Float64 reference of tests/tools/explain_ref.py against a direct conditional Student-t and its
calibration on Student-t draws; typ_tail (csrc/typicality_math.h) at D = 1 against scipy's Student-t survival function; the argument
checks of `Predictor.explain` over a stand-in worker."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package
from tools import explain_ref as E
from tools import sample_ref as SR
from tools import typicality_ref as T

HEADER = os.path.join(ROOT, "include", "dpmm_hip_explain.h")
FUNCS = ["dpmm_explain_points", "dpmm_explain_points_device"]
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


# ---------------------------------------------------------------------------------------------- the C boundary
def test_header_compiles_as_c_and_is_bound_exported_and_built(pkg, host):
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER])
    hdr = open(HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", body))) == FUNCS
    binding = importlib.import_module(pkg.__name__ + ".binding")
    assert sorted(n for n, _, _ in binding.ABI_EXPLAIN) == FUNCS
    others = (binding.ABI + binding.ABI_TENSOR + binding.ABI_SCORE + binding.ABI_RANK + binding.ABI_OVERLAP + binding.ABI_BATCHSTATS + binding.ABI_COUNTSTATS
              + binding.ABI_TYPICALITY + binding.ABI_HOLDOUT + binding.ABI_TRACE + binding.ABI_MISSING + binding.ABI_IMPUTE + binding.ABI_CSC + binding.ABI_SAMPLE
              + binding.ABI_PROJECT)
    assert not set(FUNCS) & set(n for n, _, _ in others)
    for name in ("explain_points_raw", "explain_points_into"):
        assert callable(getattr(binding.Worker, name)), name
    struct = body[body.index("typedef struct {"):body.index("} dpmm_explain_out;")]
    fields = re.findall(r"(float|int64_t|int32_t)\s*(\*?)\s*([A-Za-z_]+);", struct)
    assert [f[2] for f in fields] == [f[0] for f in binding.ExplainOut._fields_]
    ctype = {("int32_t", ""): ctypes.c_int32, ("int64_t", ""): ctypes.c_int64}
    assert [ctype.get((t, p), ctypes.c_void_p) for t, p, _ in fields] == [f[1] for f in binding.ExplainOut._fields_]
    assert [f[0] for f in binding.ExplainOut._fields_[:5]] == [f[0] for f in binding.TypicalityOut._fields_]      # the five fields of dpmm_typicality_out first
    assert int(re.search(r"#define DPMM_EXPLAIN_MAX_TOP (\d+)", hdr).group(1)) == binding.EXPLAIN_MAX_TOP == 16
    assert f"EXPLAIN_MAX_TOP = {binding.EXPLAIN_MAX_TOP};" in open(os.path.join(CSRC, "dpmm_kernels.h")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "build/explain.o" in re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "../../include/dpmm_hip_explain.h" in re.search(r"^build/dpmm_api\.o:(.*)$", mk, flags=re.M).group(1).split()
    hip = open(os.path.join(CSRC, "explain.hip")).read()
    assert "miss_rz<NT>" in hip and "miss_rty<NT>" in hip and '#include "missing_device.h"' in hip and "atomicAdd" not in hip and "__shared__" not in hip
    assert "__syncthreads" not in hip                                                    # the waves of a workgroup share nothing
    assert "void miss_rty(" in open(os.path.join(CSRC, "missing_device.h")).read()
    jl = open(os.path.join(ROOT, "julia", "gpu_explain.jl")).read()
    assert set(re.findall(r":(dpmm_[a-z0-9_]+)", jl)) == {"dpmm_explain_points"}
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for n in FUNCS:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                               # additive: the version stays
    assert callable(host.explain) and callable(host.Predictor.explain)
    assert host.Explanation._fields == ("labels", "mahalanobis", "tail", "residual", "zscore", "feature_tail", "features", "skipped", "incomplete")


# ---------------------------------------------------------------------------------------------- the reference itself
def one_cluster(D, df, seed, offdiag=None):
    """A K = 1 model of tests/tools/sample_ref.py and the worker's Float32 parameters of its predictive."""
    post, m, A, dfs = SR.niw_model(D, 1, df, seed, offdiag=offdiag)
    R = np.linalg.inv(A)                                             # Sigma^-1 = R'R, Sigma = A A'
    return post, m, A, dfs, T.worker_params(m, R, dfs)


@pytest.mark.parametrize("D", [2, 5, 64])
def test_reference_equals_a_direct_conditional_student_t(D):
    """Sigma = (R'R)^-1, feature d conditioned on the rest with numpy.linalg.solve, standardised: the t_d of the reference to 1e-9 relative
    (Sigma of these models has a condition number of a few hundred at D = 64: the two routes differ by rounding some 1e-13)."""
    rng = np.random.default_rng(D)
    for df in (4.0, 1e5):
        _, m, A, dfs, (m32, R32, df32) = one_cluster(D, df, 30 + D)
        x = (m[0] + (A[0] @ rng.standard_normal((D, 6))).T * np.array([0.3, 1, 1, 2, 5, 20])[:, None]).astype(np.float32)
        ref = E.reference(x.T, np.zeros(6, np.int64), m32, R32, df32)
        for i in range(6):
            want = E.direct_conditional(x[i], m32[0], R32[0], df32[0])
            assert np.all(np.abs(ref.t[i] - want) <= 1e-9 * np.abs(want)), (D, df, i, np.abs(ref.t[i] / want - 1).max())
            assert np.all(ref.q[i] - ref.e[i] ** 2 * (R32[0].astype(np.float64) ** 2).sum(0) >= -1e-9 * ref.q[i])      # q_-d >= 0
    if D == 2:                                                       # D = 1 collapses: t^2 = q, feature_tail = tail
        _, m, A, dfs, (m32, R32, df32) = one_cluster(1, 7.0, 31)
        x = (m[0] + A[0, 0] * np.array([[0.0], [0.5], [-3.0], [40.0]])).astype(np.float32)
        ref = E.reference(x.T, np.zeros(4, np.int64), m32, R32, df32)
        q, _, tail = T.reference(x.T, np.zeros(4, np.int64), m32, R32, df32)
        assert np.allclose(ref.t[:, 0] ** 2, q, rtol=1e-14, atol=0) and np.allclose(ref.tail[:, 0], tail, rtol=1e-6, atol=0) and ref.tail[0, 0] == 1.0


# seeds fixed here, on the CPU: each KS distance is printed and lies under the 1 % critical distance 1.63 / sqrt(n)
KS_CASES = [(2, 4.0, 21), (64, 4.0, 22), (64, 1e5, 23)]


@pytest.mark.parametrize("D,df,seed", KS_CASES)
def test_reference_feature_tails_of_student_t_draws_are_uniform(D, df, seed):
    n = 20000
    _, m, A, dfs, (m32, R32, df32) = one_cluster(D, df, 600 + seed)
    x = SR.niw_points(m, A, dfs, np.zeros(n, np.int64), np.arange(n), seed)
    ref = E.reference(x.T.astype(np.float32), np.zeros(n, np.int64), m32, R32, df32)
    for d in sorted({0, D // 2, D - 1}):
        dist = T.ks_uniform(ref.tail[:, d])
        print(f"D = {D} df = {df:g} feature {d}: KS distance {dist:.5f}, critical {1.63 / np.sqrt(n):.5f}")
        assert dist < 1.63 / np.sqrt(n)
        assert T.ks_uniform(np.clip(ref.tail[:, d] * 1.05, 0, 1)) > 1.63 / np.sqrt(n)      # the test has power: a 5 % miscalibration is seen


# ---------------------------------------------------------------------------------------------- typ_tail at D = 1
TAIL_MAIN = r"""
#include <stdio.h>
#include "typicality_math.h"
int main() {
    double q, df;
    while (scanf("%lf %lf", &q, &df) == 2) {
        int trips = 0;
        const double t = dpmm::typ_tail(q, df, 1, &trips);
        printf("%.17g %d\n", t, trips);
    }
    return 0;
}
"""


def test_typ_tail_at_one_feature_is_the_two_sided_student_t_tail(tmp_path):
    """A stand-alone host program compiled from typicality_math.h against 2 t.sf(|t|, df): relative 1e-9 wherever the reference is at least
    1e-30, on df in {1.5 .. 1e7 + 255} and t^2 in {0 .. 1e6}."""
    from scipy.stats import t as student
    src = tmp_path / "tail_main.cpp"
    src.write_text(TAIL_MAIN)
    exe = str(tmp_path / "tail_main")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", CSRC, str(src), "-o", exe])
    dfs = [1.5, 2.0, 4.0, 6.0, 19.0, 67.0, 259.0, 1000.0, 1e5, 1e5 + 255, 1e7, 1e7 + 255]
    t2 = np.concatenate([[0.0], 10.0 ** np.arange(-12.0, 6.01, 0.25), [2.0, 9.0, 144.0, 1e6]])
    grid = [(float(q), float(df)) for df in dfs for q in t2]
    out = subprocess.run([exe], input="".join(f"{q!r} {df!r}\n" for q, df in grid), capture_output=True, text=True, check=True).stdout.split("\n")
    got = np.array([float(line.split()[0]) for line in out if line])
    trips = np.array([int(line.split()[1]) for line in out if line])
    q, df = np.array(grid).T
    want = 2.0 * student.sf(np.sqrt(q), df)
    big = want >= 1e-30
    rel = np.abs(got[big] - want[big]) / want[big]
    print(f"typ_tail(., ., 1) against 2 t.sf: largest relative difference {rel.max():.3g} on {big.sum()} points, {(~big).sum()} below 1e-30, most trips {trips.max()}")
    assert len(got) == len(grid) and np.all(rel <= 1e-9) and np.all(got[~big] <= 1e-29) and np.all(got[q == 0] == 1.0)


# ---------------------------------------------------------------------------------------------- argument checks over a stand-in
def stand_in():
    from fake_worker import FakeWorker

    class Quiet(FakeWorker):
        """Takes the predictive parameters and nothing else: every refusal below comes before the worker is asked for anything."""
        asked = 0

        def set_predictive_niw(self, *a):
            pass

        def set_predictive_mult(self, *a):
            pass

        def explain_points_into(self, *a, **kw):
            Quiet.asked += 1

        def typicality_points_into(self, *a):
            Quiet.asked += 1

        def upload_points(self, *a, **kw):
            Quiet.asked += 1
    return Quiet


def niw_predictor(score, D, K, factory):
    post, _, _, _ = SR.niw_model(D, K, 9.0, 3)
    p = score.Predictor.__new__(score.Predictor)
    p._setup(0, D, 10.0, np.full(K, 50.0), post, 16, 0, factory)
    return p


def test_refusals(score, host):
    Quiet = stand_in()
    D, K = 3, 2
    X = np.zeros((D, 5), np.float32)
    mult = score.Predictor.__new__(score.Predictor)
    mult._setup(1, D, 10.0, np.full(K, 5.0), dict(alpha=np.ones((K, D), np.float32)), 16, 0, Quiet)
    with pytest.raises(ValueError, match="Multinomial.*closed-form tail"):
        mult.explain(X)
    mult.close()
    p = niw_predictor(score, D, K, Quiet)
    for bad in (0, -1, D + 1, 17, 1.5):
        with pytest.raises(ValueError, match="top"):
            p.explain(X, top=bad)
    wide = niw_predictor(score, 40, K, Quiet)
    with pytest.raises(ValueError, match=r"1\.\.16"):                # min(D, 16)
        wide.explain(np.zeros((40, 5), np.float32), top=17)
    wide.close()
    assert Quiet.asked == 0
    p.close()
    with pytest.raises(RuntimeError, match="closed"):
        p.explain(X)
    with pytest.raises(RuntimeError, match="closed"):
        p.explain(X, top=1)
    from fake_worker import FakeWorker
    q = niw_predictor(score, D, K, type("Bare", (FakeWorker,), {"set_predictive_niw": lambda self, *a: None}))
    with pytest.raises(RuntimeError, match="explain"):               # a worker without dpmm_explain_points
        q.explain(X)
    q.close()
    assert Quiet.asked == 0
