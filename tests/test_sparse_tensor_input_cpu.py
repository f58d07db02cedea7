"""torch.sparse_csc tensors as the data argument, on the CPU: recognition by host/sparse.py (a CPU tensor is the `CSC` of its three arrays),
the rejections, a CPU tensor through `fit` and a `Predictor` over stand-in workers, and the sixth header include/dpmm_hip_csc.h against
binding.ABI_CSC and the library.  The yardstick is the tuple `(colptr, rowval, nzval, (D, N))` of the same arrays."""
import ctypes
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.filterwarnings("ignore:Sparse CS[RC] tensor support is in beta state")

DTYPES = [torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.uint8, torch.int16, torch.int32, torch.int64]     # DPMM_DT_* order


def _host():
    from __graft_entry__ import load_package
    load_package()
    return importlib.import_module("dpmmsubclusters_jl_amd.host")


def _sparse():
    _host()
    return importlib.import_module("dpmmsubclusters_jl_amd.host.sparse")


def _matrix(D=9, N=14, seed=0):
    """(colptr, rowval, nzval Float32 counts) of a D x N matrix with empty columns and a full one."""
    rng = np.random.default_rng(seed)
    X = rng.poisson(0.6, size=(N, D)).astype(np.float32)
    X[0] = 0; X[N - 1] = 0; X[5] = 1 + np.arange(D) % 3
    r, c = np.nonzero(X)
    colptr = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=N), out=colptr[1:])
    return colptr, c.astype(np.int64), X[r, c], X


def _csc_tensor(colptr, rowval, nzval, shape, index=torch.int64, value=torch.float32):
    return torch.sparse_csc_tensor(torch.from_numpy(colptr).to(index), torch.from_numpy(rowval).to(index), torch.from_numpy(nzval).to(value), size=shape)


@pytest.mark.parametrize("index", [torch.int32, torch.int64])
@pytest.mark.parametrize("code", range(8))
def test_a_cpu_csc_tensor_is_the_csc_of_its_arrays(index, code):
    S = _sparse()
    cp, rv, nz, X = _matrix()
    D, N = X.shape[1], X.shape[0]
    t = _csc_tensor(cp, rv, nz, (D, N), index, DTYPES[code])
    got, want = S.as_csc(t), S.as_csc((cp, rv, nz, (D, N)))
    assert type(got) is S.CSC and got.shape == want.shape == (D, N)
    assert got.indptr.dtype == np.int64 and np.array_equal(got.indptr, want.indptr)
    for lo, hi in ((0, N), (3, 9), (N, N)):
        for a, b in zip(got.columns(lo, hi), want.columns(lo, hi)):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(got.dense_rows(0, N), X)


def test_a_csr_tensor_of_shape_n_d_comes_in_through_t():
    S = _sparse()
    cp, rv, nz, X = _matrix()
    t = torch.from_numpy(X).to_sparse_csr().t()
    assert t.layout == torch.sparse_csc and tuple(t.shape) == (X.shape[1], X.shape[0])
    got = S.as_csc(t)
    assert np.array_equal(got.indptr, cp) and np.array_equal(got.indices, rv) and np.array_equal(got.data, nz)


def test_no_canonicalisation_a_bad_tensor_is_refused_as_a_tuple_is():
    """Values that round to Float32 differently from the host conversion would show here too: bfloat16 goes through .float()."""
    S = _sparse()
    t = _csc_tensor(np.array([0, 2]), np.array([1, 0]), np.array([1.0, 2.0], np.float32), (3, 1), value=torch.bfloat16)
    got = S.as_csc(t)
    assert got.data.dtype == np.float32 and got.indices.tolist() == [1, 0]            # as given
    with pytest.raises(ValueError, match="point 0: row indices are not strictly increasing"):
        got.columns(0, 1)


def test_rejections():
    S = _sparse()
    host = _host()
    cp, rv, nz, X = _matrix()
    D, N = X.shape[1], X.shape[0]
    dense = torch.from_numpy(np.ascontiguousarray(X.T))                               # (D, N)
    batched = torch.stack([dense, dense]).to_sparse_csc()
    assert batched.layout == torch.sparse_csc and batched.ndim == 3
    bad = dict(coo=dense.to_sparse(), csr=dense.to_sparse_csr(), bsr=torch.zeros(4, 6).to_sparse_bsr((2, 2)), bsc=torch.zeros(4, 6).to_sparse_bsc((2, 2)),
               batched=batched, grad=dense.to_sparse_csc().requires_grad_(True),
               bool=_csc_tensor(cp, rv, nz, (D, N), value=torch.bool))
    hyper = host.multinomial_hyper(np.ones(D))
    from fake_worker import FakeWorker
    for name, t in bad.items():
        with pytest.raises(TypeError):
            S.as_csc(t)
        with pytest.raises(TypeError):
            host.fit(t, hyper, 10.0, iters=1, verbose=False, worker_factory=FakeWorker, nthreads=1)
    for name in ("coo", "csr", "bsr", "bsc"):
        with pytest.raises(TypeError, match="to_sparse_csc"):
            S.as_csc(bad[name])
    with pytest.raises(TypeError, match="bool"):
        S.as_csc(bad["bool"])
    S.as_csc(bad["grad"].detach())                                                    # detached: accepted
    ok = _csc_tensor(cp, rv, nz, (D, N))
    with pytest.raises(TypeError, match="Multinomial"):                               # the Gaussian prior takes no sparse data
        host.fit(ok, 10.0, iters=1, verbose=False, worker_factory=FakeWorker, nthreads=1)
    assert S.as_csc(dense) is None and S.as_csc(X) is None                            # dense input goes the dense way


def test_fit_takes_a_cpu_csc_tensor():
    host = _host()
    from fake_worker import FakeWorker
    data, _, _ = host.generate_mnmm_data(1200, 30, 3, 60, seed=4, sparse=True)
    cp, rv, nz, shape = data
    hyper = host.multinomial_hyper(np.ones(30))
    kw = dict(iters=25, seed=9, burnout=5, verbose=False, worker_factory=FakeWorker, nthreads=1)
    ref = host.fit(data, hyper, 10.0, **kw)
    for index, value in ((torch.int64, torch.float32), (torch.int32, torch.uint8), (torch.int32, torch.bfloat16)):
        got = host.fit(_csc_tensor(np.asarray(cp), np.asarray(rv), np.asarray(nz, np.float32), shape, index, value), hyper, 10.0, **kw)
        assert isinstance(got[0], np.ndarray) and np.array_equal(ref[0], got[0]) and np.array_equal(ref[7], got[7]) and ref[6] == got[6]
    assert ref[6][-1] >= 2                                                            # (the chain did something)


def test_a_predictor_takes_a_cpu_csc_tensor():
    from test_score_cpu import StandIn, model
    _host()
    score = importlib.import_module("dpmmsubclusters_jl_amd.host.score")
    cp, rv, nz, X = _matrix(D=5, N=23, seed=3)
    with score.Predictor(model(1, 5, 4), capacity=10, worker_factory=StandIn) as p:     # two full slabs and a short one
        want = p.predict((cp, rv, nz, (5, 23)))
        got = p.predict(_csc_tensor(cp, rv, nz, (5, 23), torch.int32, torch.int16))
        dense = p.predict(np.ascontiguousarray(X.T))
    for a, b, c in zip(want, got, dense):
        assert isinstance(b, np.ndarray) and np.array_equal(a, b) and np.array_equal(a, c)


# ---------------------------------------------------------------------------------------------- the sixth header
HEADER = os.path.join(ROOT, "include", "dpmm_hip_csc.h")


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", src)))


def test_csc_header_binding_and_library_agree():
    from __graft_entry__ import load_package
    pkg = load_package()
    pkg.build_library()
    binding = importlib.import_module("dpmmsubclusters_jl_amd.binding")
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER])
    names = _declared()
    assert names == ["dpmm_upload_points_csc_device"] == sorted(n for n, _, _ in binding.ABI_CSC)
    for other in (binding.ABI, binding.ABI_TENSOR, binding.ABI_SCORE):                # additive: nothing moved, nothing added elsewhere
        assert not set(names) & set(n for n, _, _ in other)
    lib = ctypes.CDLL(pkg.lib_path())
    for n in names:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3
    assert hasattr(binding.Worker, "upload_points_csc_device") and hasattr(binding.Worker, "upload_points_csc_tensor")
    mk = open(os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc", "Makefile")).read()
    assert "build/csc_io.o" in mk and re.search(r"^build/dpmm_api\.o:.*dpmm_hip_csc\.h", mk, flags=re.M)


def test_the_csc_call_refuses_without_a_device():
    """No CPU fallback: DPMM_ENODEVICE without a device; with one, a null context is a bad argument."""
    _host()
    binding = importlib.import_module("dpmmsubclusters_jl_amd.binding")
    lib = binding.load_library()
    want = -1 if torch.cuda.is_available() else -2
    buf = ctypes.c_void_p(0)
    assert lib.dpmm_upload_points_csc_device(None, buf, binding.DT_I64, buf, buf, binding.DT_F32, 0, 0) == want
    assert (b"no HIP device" in lib.dpmm_last_error(None)) == (want == -2)
