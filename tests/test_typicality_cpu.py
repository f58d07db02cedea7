"""CPU-side checks of the calibrated outlier scores (include/dpmm_hip_typicality.h): the header compiles as C, its functions are bound,
exported and built from csrc/typicality.hip; the Float64 reference of tests/tools/typicality_ref.py against scipy's F distribution and its
calibration on Student-t draws; the argument checks of `Predictor.typicality` and of `min_tail` over a stand-in worker."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package
from tools import sample_ref as SR
from tools import typicality_ref as T

HEADER = os.path.join(ROOT, "include", "dpmm_hip_typicality.h")
FUNCS = ["dpmm_batchstats_set_min_tail", "dpmm_typicality_points", "dpmm_typicality_points_device"]


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
    assert sorted(n for n, _, _ in binding.ABI_TYPICALITY) == FUNCS
    others = (binding.ABI + binding.ABI_TENSOR + binding.ABI_SCORE + binding.ABI_RANK + binding.ABI_OVERLAP + binding.ABI_BATCHSTATS + binding.ABI_COUNTSTATS
              + binding.ABI_TRACE + binding.ABI_MISSING + binding.ABI_IMPUTE + binding.ABI_CSC + binding.ABI_SAMPLE + binding.ABI_PROJECT)
    assert not set(FUNCS) & set(n for n, _, _ in others)
    for name in ("typicality_points_raw", "typicality_points_into", "batchstats_set_min_tail"):
        assert callable(getattr(binding.Worker, name)), name
    struct = body[body.index("typedef struct {"):body.index("} dpmm_typicality_out;")]
    assert re.findall(r"\*\s*([A-Za-z_]+);", struct) == [f[0] for f in binding.TypicalityOut._fields_]
    assert re.findall(r"(float|int64_t)\s*\*", struct) == ["int64_t", "float", "float", "int64_t", "int64_t"]
    csrc = os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "build/typicality.o" in re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "../../include/dpmm_hip_typicality.h" in re.search(r"^build/dpmm_api\.o:(.*)$", mk, flags=re.M).group(1).split()
    hip = open(os.path.join(csrc, "typicality.hip")).read()
    assert "miss_rz<NT>" in hip and '#include "missing_device.h"' in hip and "atomicAdd(&A.q" not in hip and "atomicAdd(&A.tail" not in hip
    assert "miss_rz<NT>" in open(os.path.join(csrc, "missing.hip")).read()                  # one copy of y = R z, shared
    jl = open(os.path.join(ROOT, "julia", "gpu_typicality.jl")).read()
    assert set(re.findall(r":(dpmm_[a-z0-9_]+)", jl)) <= set(FUNCS) | {"dpmm_last_error"}
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for n in FUNCS:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                               # additive: the version stays
    assert callable(host.typicality) and callable(host.Predictor.typicality)
    assert host.Typicality._fields == ("labels", "mahalanobis", "tail", "skipped", "incomplete")


# ---------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("D", [2, 17, 64, 256])
def test_reference_agrees_with_the_F_distribution(D):
    """tail(q) = P(F(D, df) >= q / D): two routes through scipy (betainc, and the F survival function) on the same Float64 inputs.
    Tolerance: both routes subtract log-gamma values of size (df / 2) log(df / 2) -- 7.7e7 at df = 1e7 -- rounded to 2^-53 relative each:
    up to four such roundings, 3.4e-8 in the logarithm of the result; 1e-7 covers it and is a tenth of the Float32 allowance of the GPU test."""
    from scipy.stats import f
    rng = np.random.default_rng(D)
    for df in (4.0, 300.0, 1e5, 1e7):
        q = np.concatenate([D * np.exp(rng.normal(0, 0.7, 200)), [0.0, 1e-3, 1.0, 100.0, 1e4]])
        got, want = T.tail_of(q, df, D), f.sf(q / D, D, df)
        big = want >= 1e-200
        assert np.all(np.abs(got[big] - want[big]) <= 1e-7 * want[big]) and np.all(got[~big] <= 1e-199), (D, df)
        assert got[200] == 1.0


def one_cluster(D, df, seed):
    """A K = 1 model of tests/tools/sample_ref.py and the worker's Float32 parameters of its predictive."""
    post, m, A, dfs = SR.niw_model(D, 1, df, seed)
    R = np.linalg.inv(A)                                             # Sigma^-1 = R'R, Sigma = A A'
    return post, m, A, dfs, T.worker_params(m, R, dfs)


# seeds fixed here, on the CPU: each case's KS distance is printed and lies under the 1 % critical distance 1.63 / sqrt(n)
KS_CASES = [(2, 4.0, 11), (2, 1e5, 12), (64, 4.0, 13), (64, 1e5, 14)]


@pytest.mark.parametrize("D,df,seed", KS_CASES)
def test_reference_tails_of_student_t_draws_are_uniform(D, df, seed):
    n = 20000
    post, m, A, dfs, (m32, R32, df32) = one_cluster(D, df, 500 + seed)
    x = SR.niw_points(m, A, dfs, np.zeros(n, np.int64), np.arange(n), seed)
    q, _, tail = T.reference(x.T.astype(np.float32), np.zeros(n, np.int64), m32, R32, df32)
    d = T.ks_uniform(tail)
    print(f"D = {D} df = {df:g}: KS distance {d:.5f}, critical {1.63 / np.sqrt(n):.5f}, mean q / D {q.mean() / D:.4f}")
    assert d < 1.63 / np.sqrt(n)
    assert T.ks_uniform(np.clip(tail * 1.05, 0, 1)) > 1.63 / np.sqrt(n)      # the test has power: a 5 % miscalibration is seen


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

        def batchstats_begin(self, *a):
            Quiet.asked += 1

        def typicality_points_into(self, *a):
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
        mult.typicality(X)
    mult.close()
    p = niw_predictor(score, D, K, Quiet)
    for bad in (0.0, -0.1, 1.0000001, float("nan"), float("inf")):
        for call in (p.statistics, p.absorb):
            with pytest.raises(ValueError, match="min_tail"):
                call(X, min_tail=bad)
    with pytest.raises(ValueError, match="min_tail"):
        p.statistics(X, min_logdens=-5.0, min_tail=2.0)
    assert Quiet.asked == 0
    with pytest.raises(RuntimeError, match="tail"):                  # a worker without dpmm_batchstats_set_min_tail
        p.statistics(X, min_tail=0.5)
    assert Quiet.asked == 0
    p.close()
    with pytest.raises(RuntimeError, match="closed"):
        p.typicality(X)
    with pytest.raises(RuntimeError, match="closed"):
        p.statistics(X, min_tail=0.5)
    from fake_worker import FakeWorker
    q = niw_predictor(score, D, K, type("Bare", (FakeWorker,), {"set_predictive_niw": lambda self, *a: None}))
    with pytest.raises(RuntimeError, match="typicality"):            # a worker without dpmm_typicality_points
        q.typicality(X)
    q.close()
