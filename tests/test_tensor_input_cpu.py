"""torch tensors as the data argument, on the CPU: the description of a tensor (host/tensors.py), the rejections, CPU tensors through
the public entry points over the oracle-backed stand-in worker, the numpy statement of what the device ingest computes (`ref_ingest`,
which tests/test_gpu_tensor_io.py imports), and the fourth header include/dpmm_hip_tensor.h against binding.ABI_TENSOR and the library.
Every comparison is bit for bit: a conversion to Float32 has one right answer."""
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

DTYPES = [torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.uint8, torch.int16, torch.int32, torch.int64]     # DPMM_DT_* order
ITEMSIZE = [2, 2, 4, 8, 1, 2, 4, 8]


def _host():
    from __graft_entry__ import load_package
    load_package()
    return importlib.import_module("dpmmsubclusters_jl_amd.host")


def _tensors():
    _host()
    return importlib.import_module("dpmmsubclusters_jl_amd.host.tensors")


# ---------------------------------------------------------------------------------------------- the ingest semantics, in numpy
_NP_STORAGE = [np.uint16, np.uint16, np.float32, np.float64, np.uint8, np.int16, np.int32, np.int64]      # float16 / bfloat16 as their bits


def storage_of(t):
    """The whole storage behind tensor `t` as a 1-D numpy array of `_NP_STORAGE[code]` (16-bit floats as bits), and the tensor's offset into it
    in elements.  `t` may live anywhere; the copy is on the host."""
    code = DTYPES.index(t.dtype)
    n_el = t.untyped_storage().nbytes() // ITEMSIZE[code]
    flat = torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage(), 0, (n_el,), (1,)).cpu()
    if code < 2:
        flat = flat.view(torch.int16)
    return flat.numpy().view(_NP_STORAGE[code]), int(t.storage_offset())


def ref_ingest(storage, dtype, strides, n, D, offset=0, nan_to_zero=False):
    """What dpmm_upload_points_strided_device leaves in the context: [n][ldx] float32, ldx = roundup(D, 4), element (i, d) = the source element
    storage[offset + i * strides[0] + d * strides[1]] of DPMM_DT_* type `dtype` rounded to Float32 to nearest even, pad columns 0.
    `storage`: 1-D numpy array of the element type; float16 / bfloat16 as uint16 bit patterns."""
    sp, sf = int(strides[0]), int(strides[1])
    ldx = (D + 3) // 4 * 4
    out = np.zeros((n, ldx), np.float32)
    if n == 0:
        return out
    idx = offset + np.arange(n, dtype=np.int64)[:, None] * sp + np.arange(D, dtype=np.int64)[None, :] * sf
    raw = np.asarray(storage)[idx]
    if dtype == 0:
        val = raw.astype(np.uint16).view(np.float16).astype(np.float32)                  # exact: every binary16 value is a Float32 value
    elif dtype == 1:
        val = (raw.astype(np.uint32) << np.uint32(16)).view(np.float32)                  # bfloat16 = the upper half of a Float32
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            val = raw.astype(np.float32)                                                 # IEEE conversion: round to nearest even
    if nan_to_zero:
        val = np.where(np.isnan(val), np.float32(0), val)
    out[:, :D] = val
    return out


def same_bits(a, b):
    """Equal bit for bit, NaN payloads aside (NaN must meet NaN)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def special_values(dtype, count, seed=0):
    """`count` values of a torch dtype that exercise the conversion: for the float types +-0, +-Inf, NaN, subnormals, extremes and (Float64)
    values that round at Float32's 24th bit, ties included; for the integer types the extremes and |v| > 2^24; the rest random."""
    rng = np.random.default_rng(seed)
    if dtype in (torch.float16, torch.bfloat16):
        bits = rng.integers(0, 1 << 16, count, dtype=np.int64)
        fixed = [0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0x0001, 0x8001, 0x03FF, 0x0400, 0x7BFF, 0xFBFF, 0x3C00] if dtype == torch.float16 else \
                [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x0001, 0x8001, 0x007F, 0x0080, 0x7F7F, 0xFF7F, 0x3F80]
        bits[:min(count, len(fixed))] = fixed[:count]
        return torch.from_numpy(bits.astype(np.uint16).view(np.int16)).view(dtype)
    if dtype == torch.float32:
        v = rng.standard_normal(count).astype(np.float32)
        fixed = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, 3.4028235e38, -3.4028235e38], np.float32)
        v[:min(count, fixed.size)] = fixed[:count]
        return torch.from_numpy(v)
    if dtype == torch.float64:
        v = rng.standard_normal(count) * 10.0 ** rng.integers(-3, 4, count)
        fixed = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1 + 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50, 1 + 3 * 2.0 ** -24, 1 + 2.0 ** -23 - 2.0 ** -52,
                          -(1 + 2.0 ** -24), 16777217.0, 16777219.0, 1e39, -1e39, 3.4028235677973366e38, 1e-40, -1e-40, 1e-46, 8e-46, 2.0 ** -150,
                          1.1754943508222875e-38, 0.1, 1.0 / 3.0])
        v[:min(count, fixed.size)] = fixed[:count]
        return torch.from_numpy(v)
    info = torch.iinfo(dtype)
    v = rng.integers(max(info.min, -(1 << 40)), min(info.max, 1 << 40), count, dtype=np.int64, endpoint=True)
    fixed = [0, 1, info.max, info.min, info.max - 1, 255 if info.max >= 255 else info.max]
    if info.max > (1 << 25):
        fixed += [(1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1, (1 << 25) + 2, (1 << 25) + 6, info.max - 64]
    if dtype == torch.int64:
        fixed += [(1 << 53) + 1, (1 << 62) + (1 << 38), (1 << 62) + (1 << 38) + 1, -(1 << 62) - (1 << 38), (1 << 40) + (1 << 16), (1 << 40) + (1 << 16) + 1]
    v[:min(count, len(fixed))] = fixed[:count]
    return torch.from_numpy(v).to(dtype)


@pytest.mark.parametrize("code", range(8))
def test_ref_ingest_is_the_float_conversion(code):
    dtype = DTYPES[code]
    n, D = 37, 5
    t = special_values(dtype, 4 * D * n + 3, seed=code)[3:].reshape(4 * D, n)      # (storage offset 3)
    views = dict(contiguous=t[:D], columns=t[:D, 5:31], steps=t[::3, ::2][:D], expanded=t[:D, 7:8].expand(D, 11), transposed=t[:n, :D].T)
    for name, v in views.items():
        st, off = storage_of(v)
        got = ref_ingest(st, code, (v.stride(1), v.stride(0)), v.shape[1], D, offset=off)
        want = v.float().numpy().T
        assert same_bits(got[:, :D], want), name
        assert not got[:, D:].any(), name
    st, off = storage_of(t)
    z = ref_ingest(st, code, (t.stride(1), t.stride(0)), n, 4 * D, offset=off, nan_to_zero=True)
    assert same_bits(z, torch.nan_to_num(t.float(), nan=0.0, posinf=float("inf"), neginf=float("-inf")).numpy().T)
    assert ref_ingest(st, code, (1, n), 0, D).shape == (0, 8)


def test_the_special_values_hit_the_hard_cases():
    f64 = special_values(torch.float64, 64)
    f32 = f64.float().numpy()
    assert f32[5] == 1.0 and f32[6] == np.float32(1 + 2.0 ** -23) and f32[7] == np.float32(1 + 2.0 ** -22)      # ties to even; above a tie
    assert np.isinf(f32[12]) and 0 < f32[15] < 1.2e-38 and f32[17] == 0 and f32[18] == np.float32(1e-45) and f32[19] == 0        # overflow; subnormal results
    i64 = special_values(torch.int64, 64)
    assert (i64.abs() > (1 << 24)).sum() > 8 and int(i64[6].float()) != int(i64[6])                                      # values Float32 cannot hold
    h = special_values(torch.float16, 64).float().numpy()
    assert h[5] == 2.0 ** -24 and h[7] == 1023 * 2.0 ** -24                                                          # binary16 subnormals


# ---------------------------------------------------------------------------------------------- the description of a tensor
def _element(desc, lo, i, d):
    """The element (point lo + i, feature d) read through the description's pointer arithmetic (the tensor lives on the host here)."""
    ct = {1: ctypes.c_uint8, 2: ctypes.c_uint16, 4: ctypes.c_uint32, 8: ctypes.c_uint64}[desc.itemsize]
    return ct.from_address(desc.shard_ptr(lo) + (i * desc.stride_point + d * desc.stride_feature) * desc.itemsize).value


def _bits(t):
    code = DTYPES.index(t.dtype)
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[ITEMSIZE[code]]
    return int(t.view(view)) & ((1 << (8 * ITEMSIZE[code])) - 1)


@pytest.mark.parametrize("code", range(8))
def test_descriptor_strides_dtype_and_shard_offset(code):
    T = _tensors()
    dtype = DTYPES[code]
    D, N = 6, 41
    base = special_values(dtype, 3 * D * 2 * N, seed=10 + code)
    wide = base.reshape(3 * D, 2 * N)
    cases = dict(
        contiguous=(wide[:D, :N].contiguous(), (1, N)),
        transposed=(base[:N * D].reshape(N, D).T, (D, 1)),
        column_slice=(wide[:D, 7:7 + N], (1, 2 * N)),
        steps=(wide[::2, ::3][:D, :N // 2], (3, 4 * N)),
        expanded=(wide[:D, 3:4].expand(D, N), (0, 2 * N)),
    )
    for name, (t, (sp, sf)) in cases.items():
        desc = T.describe(t)
        assert desc.dtype == code and desc.itemsize == ITEMSIZE[code], name
        assert desc.shape == tuple(t.shape) and (desc.stride_point, desc.stride_feature) == (sp, sf), name
        assert desc.shard_ptr(0) == t.data_ptr() and desc.tensor is t, name
        n = t.shape[1]
        lo = n // 2 + 1                                                  # an odd split: the second shard of a two-rank run
        assert desc.shard_ptr(lo) - desc.shard_ptr(0) == lo * sp * ITEMSIZE[code], name
        for i, d in ((0, 0), (n - lo - 1, D - 1), (1, 2)):
            assert _element(desc, lo, i, d) == _bits(t[d, lo + i]), (name, i, d)
    assert T.as_device_points(cases["contiguous"][0]) is None           # a CPU tensor takes the host path
    assert T.as_device_points(np.zeros((2, 3), np.float32)) is None and T.as_device_points([[1.0, 2.0]]) is None


def test_rejections():
    T = _tensors()
    host = _host()
    ok = torch.zeros(3, 8)
    bad = [torch.zeros(3, 8, dtype=torch.bool), torch.zeros(3, 8, dtype=torch.complex64), torch.zeros(3, 8, dtype=torch.int8),
           torch.quantize_per_tensor(ok, 0.1, 0, torch.quint8), ok.to_sparse(), ok.to_sparse_csr(), ok.clone().requires_grad_(True),
           torch.zeros(8), torch.zeros(2, 3, 8)]
    for t in bad:
        with pytest.raises(TypeError):
            T.as_device_points(t)
        with pytest.raises(TypeError):
            host.fit(t, 10.0, iters=1, verbose=False)
    with pytest.raises(TypeError, match="bool"):
        T.describe(bad[0])
    with pytest.raises(TypeError, match="complex64"):
        T.describe(bad[1])
    T.describe(bad[6].detach())                                          # detached: accepted

    class OnDevice1:                                                     # what resolve_device reads of a description
        device_index, torch_device = 1, "cuda:1"
    assert T.resolve_device(OnDevice1, None) == 1 and T.resolve_device(OnDevice1, 1) == 1
    assert T.resolve_device(OnDevice1, "cuda:1") == 1 and T.resolve_device(OnDevice1, torch.device("cuda", 1)) == 1
    for dev in (0, "cuda:0", torch.device("cuda", 0)):
        with pytest.raises(ValueError, match="disagrees"):
            T.resolve_device(OnDevice1, dev)


# ---------------------------------------------------------------------------------------------- CPU tensors through fit
def _fit(host, data, **kw):
    from fake_worker import FakeWorker
    res = host.fit(data, 10.0, iters=25, seed=17, burnout=5, verbose=False, worker_factory=FakeWorker, nthreads=1, **kw)
    return res[0], res[7], np.array(res[6])


def test_fit_takes_cpu_tensors():
    """A bfloat16 tensor (numpy has no such type), a Float32 tensor that is a transposed view, Float16 and Int32: the chain of the
    Float32 host array of the same values, bit for bit.  Ground truth may be a tensor."""
    host = _host()
    x, y, _, _ = host.generate_gaussian_data(1500, 2, 4, 60.0, seed=3)
    xt = torch.from_numpy(x)
    forms = dict(bf16=xt.to(torch.bfloat16), f32_T=xt.T.contiguous().T, f16=xt.to(torch.float16), i32=(xt * 8).to(torch.int32),
                 f64_steps=torch.from_numpy(np.repeat(x.astype(np.float64), 2, axis=1))[:, ::2])
    assert not forms["f32_T"].is_contiguous() and not forms["f64_steps"].is_contiguous()
    for name, t in forms.items():
        ref = _fit(host, t.float().numpy())
        got = _fit(host, t)
        for a, b in zip(ref, got):
            assert isinstance(b, np.ndarray) and np.array_equal(a, b), name
        assert ref[2][-1] >= 2, name                                      # (the chain did something)
    from fake_worker import FakeWorker
    a = host.fit(forms["bf16"], 10.0, iters=12, seed=3, burnout=3, verbose=False, worker_factory=FakeWorker, nthreads=1, gt=torch.from_numpy(y))
    b = host.fit(forms["bf16"].float().numpy(), 10.0, iters=12, seed=3, burnout=3, verbose=False, worker_factory=FakeWorker, nthreads=1, gt=y)
    assert np.array_equal(a[0], b[0]) and a[4] == b[4] and len(a[4]) == 12


def test_count_tensor_through_the_multinomial_prior():
    host = _host()
    from fake_worker import FakeWorker
    x, _, _ = host.generate_mnmm_data(1200, 30, 3, 60, seed=4)
    hyper = host.multinomial_hyper(np.ones(30))
    kw = dict(iters=20, seed=9, burnout=5, verbose=False, worker_factory=FakeWorker, nthreads=1)
    ref = host.dp_parallel(x, hyper, 10.0, **kw)
    for t in (torch.from_numpy(x).to(torch.uint8), torch.from_numpy(x).to(torch.int64), torch.from_numpy(np.ascontiguousarray(x.T)).to(torch.int16).T):
        got = host.dp_parallel(t, hyper, 10.0, **kw)
        assert np.array_equal(ref[0].labels, got[0].labels) and np.array_equal(ref[0].labels_subcluster, got[0].labels_subcluster)
        assert ref[4] == got[4]


# ---------------------------------------------------------------------------------------------- the fourth header
HEADER = os.path.join(ROOT, "include", "dpmm_hip_tensor.h")


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", src)))


def test_tensor_header_binding_and_library_agree():
    from __graft_entry__ import load_package
    pkg = load_package()
    pkg.build_library()
    binding = importlib.import_module("dpmmsubclusters_jl_amd.binding")
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER])
    names = _declared()
    assert len(names) == 5 and names == sorted(n for n, _, _ in binding.ABI_TENSOR)
    assert not set(names) & set(n for n, _, _ in binding.ABI)            # additive: nothing moved out of the three worker headers
    lib = ctypes.CDLL(pkg.lib_path())
    for n in names:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3
    src = open(HEADER).read()
    for code, name in enumerate(("F16", "BF16", "F32", "F64", "U8", "I16", "I32", "I64")):
        assert re.search(rf"DPMM_DT_{name} = {code}\b", src) and getattr(binding, "DT_" + name) == code
    # the dependency line of the object that includes it
    mk = open(os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc", "Makefile")).read()
    assert "build/tensor_io.o" in mk and re.search(r"^build/dpmm_api\.o:.*dpmm_hip_tensor\.h", mk, flags=re.M)


def test_tensor_calls_refuse_without_a_device():
    """No CPU fallback: without a device there is no context, and the calls say DPMM_ENODEVICE (with one, a null context is a bad argument)."""
    _host()
    binding = importlib.import_module("dpmmsubclusters_jl_amd.binding")
    lib = binding.load_library()
    want = -1 if torch.cuda.is_available() else -2
    buf = ctypes.c_void_p(0)
    assert lib.dpmm_upload_points_strided_device(None, buf, binding.DT_F32, 1, 1, 0) == want
    assert lib.dpmm_get_points_device(None, buf, 4) == want
    assert lib.dpmm_get_labels_device(None, buf, buf) == want
    assert lib.dpmm_set_labels_device(None, buf, buf) == want
    assert lib.dpmm_predict_points_device(None, buf, buf) == want
    assert (b"no HIP device" in lib.dpmm_last_error(None)) == (want == -2)
