"""GPU tests of sparse points out of device memory (dpmm_upload_points_csc_device, csrc/csc_io.hip; include/dpmm_hip_csc.h).  The yardstick
is the existing host call dpmm_upload_points_csc on the same matrix with the values cast on the host (`astype(float32)`): every comparison
is bit for bit -- a conversion to Float32, a check and a compaction have one right answer.  Shapes: D = 300, n = 5003 -- n is no multiple of
the 64-point run or the 256-thread workgroup, and spans three tiles of the offsets' scan."""
import importlib

import numpy as np
import pytest
import torch

from test_gpu_mult import make_problem
from test_sparse_input_cpu import _topics

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:Sparse CS[RC] tensor support is in beta state")]

DTYPES = [torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.uint8, torch.int16, torch.int32, torch.int64]     # DPMM_DT_* order
D, N, K = 300, 5003, 5
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def host(pkg):
    return importlib.import_module("dpmmsubclusters_jl_amd.host")


@pytest.fixture(scope="module")
def binding(pkg):
    return importlib.import_module(pkg.__name__ + ".binding")


def _build_matrix():
    """colptr, rowval (Int64, 0-based) and values (Float64) of the D x N matrix of the module docstring's cases: empty columns at 0, N - 1 and
    [2000, 2300); columns of 1, 255, 256, 257 and D entries; explicit zeros as first, last and only entry; 1e-50 (0 as Float32); a value that
    rounds (1 + 2^-30)."""
    rng = np.random.default_rng(7)
    length = rng.integers(0, 24, N)
    length[0] = length[N - 1] = 0
    length[2000:2300] = 0
    length[[10, 11, 12, 13, 14]] = [1, 255, 256, 257, D]
    length[[20, 21, 22, 23, 24]] = [1, 5, 5, 5, 5]
    colptr = np.zeros(N + 1, np.int64)
    np.cumsum(length, out=colptr[1:])
    rowval = np.concatenate([np.sort(rng.choice(D, int(m), replace=False)) for m in length]).astype(np.int64)
    val = rng.integers(1, 6, rowval.size).astype(np.float64)
    val[colptr[20]] = 0.0                       # the only entry
    val[colptr[21]] = 0.0                       # the first
    val[colptr[22 + 1] - 1] = 0.0               # the last
    val[colptr[23] + 1] = 1e-50
    val[colptr[24] + 2] = 1.0 + 2.0 ** -30
    return colptr, rowval, val


MATRIX = _build_matrix()
PARAMS = make_problem(D, 8, K, 10, seed=1)
_rng = np.random.default_rng(11)
LABELS, SUB = _rng.integers(1, K + 1, N), _rng.integers(1, 3, N)


def _values_as(code):
    """The matrix's values in element type `code` (a torch CPU tensor), and those cast to Float32 on the host."""
    t = torch.from_numpy(MATRIX[2]).to(DTYPES[code])
    return t, t.float().numpy() if code == 1 else t.numpy().astype(np.float32)


def _points(wk):
    out = torch.empty((wk.n, wk.D), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    wk.get_points_device(out.data_ptr(), wk.D)
    return out.cpu().numpy()


def _state(wk, lo=0, hi=N):
    """What the kernels downstream make of the points in force: the points, the statistics and the debug table under one set of parameters."""
    pts = _points(wk)
    wk.set_labels(LABELS[lo:hi], SUB[lo:hi])
    wk.set_num_clusters(K)
    st = wk.suffstats_packed().copy()
    wk.set_params_mult(PARAMS["logp"], PARAMS["lr"], PARAMS["w"])
    return pts, st, wk.debug_loglik().copy()


def _assert_same(a, b):
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def _device_arrays(index, base, values):
    cp = torch.from_numpy(MATRIX[0] + base).to(index).to(DEV)
    rv = torch.from_numpy(MATRIX[1] + base).to(index).to(DEV)
    nz = values.to(DEV)
    torch.cuda.synchronize()
    return cp, rv, nz


_IDX = {torch.int32: 6, torch.int64: 7}
_host_state = {}


def _host_reference(pkg, code):
    """The host upload of the values cast on the host: computed once per element type, never changed."""
    if code not in _host_state:
        wk = pkg.Worker(pkg.PRIOR_MULT, D, N, device=0, seed=3)
        wk.upload_points_csc(MATRIX[0], MATRIX[1], _values_as(code)[1])
        _host_state[code] = _state(wk)
        wk.close()
    return _host_state[code]


# ---- 6. ingest parity
@pytest.mark.parametrize("code", range(8))
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("index", [torch.int32, torch.int64])
def test_ingest_equals_the_host_upload(pkg, index, base, code):
    want = _host_reference(pkg, code)
    cp, rv, nz = _device_arrays(index, base, _values_as(code)[0])
    wk = pkg.Worker(pkg.PRIOR_MULT, D, N, device=0, seed=3)
    wk.upload_points_csc_device(cp.data_ptr(), _IDX[index], rv.data_ptr(), nz.data_ptr(), code, rv.numel(), base)
    got = _state(wk)
    wk.close()
    _assert_same(got, want)
    dense = np.zeros((N, D), np.float32)
    dense[np.repeat(np.arange(N), np.diff(MATRIX[0])), MATRIX[1]] = _values_as(code)[1]
    assert np.array_equal(got[0], dense) and got[0][14].all() and not got[0][20].any()


def test_dense_and_sparse_uploads_of_either_kind_follow_each_other(pkg):
    cp, rv, nz = _device_arrays(torch.int64, 0, _values_as(2)[0])
    wk = pkg.Worker(pkg.PRIOR_MULT, D, N, device=0, seed=3)
    wk.set_labels(LABELS, SUB); wk.set_num_clusters(K)
    wk.set_params_mult(PARAMS["logp"], PARAMS["lr"], PARAMS["w"])             # parameters in force are re-packed by every upload
    want = _host_reference(pkg, 2)
    wk.upload_points(np.ones((N, D), np.float32))
    wk.upload_points_csc_device(cp.data_ptr(), 7, rv.data_ptr(), nz.data_ptr(), 2, rv.numel(), 0)
    assert np.array_equal(wk.debug_loglik(), want[2])
    wk.upload_points_csc(MATRIX[0][:N + 1] * 0, MATRIX[1][:0], np.zeros(0, np.float32))      # (all points empty)
    assert not _points(wk).any()
    wk.upload_points_csc_device(cp.data_ptr(), 7, rv.data_ptr(), nz.data_ptr(), 2, rv.numel(), 0)
    assert np.array_equal(wk.debug_loglik(), want[2]) and np.array_equal(_points(wk), want[0])
    wk.upload_points(want[0])
    np.testing.assert_allclose(wk.debug_loglik(), want[2], rtol=1e-5, atol=1e-3)
    wk.close()


# ---- 7. shards and slabs of one tensor
def test_two_shards_of_one_tensor_and_an_empty_shard(pkg, host):
    S = importlib.import_module(pkg.__name__ + ".host.sparse")
    vals, f32 = _values_as(3)
    t = torch.sparse_csc_tensor(torch.from_numpy(MATRIX[0]).to(torch.int32), torch.from_numpy(MATRIX[1]).to(torch.int32), vals, size=(D, N)).to(DEV)
    desc = S.as_csc(t)
    assert isinstance(desc, S.DeviceCSC) and desc.shape == (D, N) and desc.nnz_extent == MATRIX[1].size
    whole = S.CSC(MATRIX[0], MATRIX[1], f32, (D, N))
    desc.synchronize()
    for lo, hi in ((0, 2500), (2500, N), (2100, 2200)):
        a = pkg.Worker(pkg.PRIOR_MULT, D, hi - lo, first_index=lo, device=0, seed=3)
        b = pkg.Worker(pkg.PRIOR_MULT, D, hi - lo, first_index=lo, device=0, seed=3)
        a.upload_points_csc_tensor(desc, lo, hi)
        b.upload_points_csc(*whole.columns(lo, hi))
        _assert_same(_state(a, lo, hi), _state(b, lo, hi))
        a.close(); b.close()
    e = pkg.Worker(pkg.PRIOR_MULT, D, 0, first_index=N, device=0, seed=3)
    e.upload_points_csc_tensor(desc, N, N)
    e.upload_points_csc_device(0, 7, 0, 0, 2, 0, 0)
    e.set_params_mult(PARAMS["logp"], PARAMS["lr"], PARAMS["w"])
    e.init_labels(K, 1); e.sweep(1)
    assert not e.suffstats_packed().any()
    e.close()


# ---- 8. refused before anything is launched
def test_refusals_before_any_launch(pkg):
    cp, rv, nz = _device_arrays(torch.int64, 0, _values_as(2)[0])
    wk = pkg.Worker(pkg.PRIOR_MULT, D, N, device=0, seed=3)
    wk.upload_points_csc_device(cp.data_ptr(), 7, rv.data_ptr(), nz.data_ptr(), 2, rv.numel(), 0)
    before = _points(wk)
    hostmem = np.zeros(N + 1, np.int64)
    ext = rv.numel()
    good = dict(colptr_ptr=cp.data_ptr(), index_dtype=7, rowval_ptr=rv.data_ptr(), nzval_ptr=nz.data_ptr(), value_dtype=2, nnz_extent=ext, index_base=0)
    cases = [(dict(colptr_ptr=hostmem.ctypes.data), "d_colptr"), (dict(rowval_ptr=hostmem.ctypes.data), "d_rowval"), (dict(nzval_ptr=0), "d_nzval is null"),
             (dict(colptr_ptr=0), "d_colptr is null"), (dict(rowval_ptr=4096), "d_rowval"), (dict(colptr_ptr=cp.data_ptr() + 4), "d_colptr is not aligned"),
             (dict(nnz_extent=1 << 40), "d_rowval: the call addresses"), (dict(index_dtype=2), "index_dtype"), (dict(value_dtype=8), "value_dtype"),
             (dict(value_dtype=-1), "value_dtype"), (dict(index_base=2), "index_base"), (dict(nnz_extent=-1), "nnz_extent")]
    for change, what in cases:
        with pytest.raises(pkg.DpmmError, match=what) as ei:
            wk.upload_points_csc_device(**{**good, **change})
        assert ei.value.code == -1, what
        assert np.array_equal(_points(wk), before), what
    wk.close()
    niw = pkg.Worker(pkg.PRIOR_NIW, 4, 10, device=0, seed=1)
    with pytest.raises(pkg.DpmmError, match="Multinomial") as ei:
        niw.upload_points_csc_device(cp.data_ptr(), 7, rv.data_ptr(), nz.data_ptr(), 2, ext, 0)
    assert ei.value.code == -1
    niw.close()
    big = pkg.Worker(pkg.PRIOR_MULT, 65537, 10, device=0, seed=1)
    with pytest.raises(pkg.DpmmError) as ei:
        big.upload_points_csc_device(cp.data_ptr(), 7, rv.data_ptr(), nz.data_ptr(), 2, ext, 0)
    assert ei.value.code == -5
    big.close()


# ---- 9. refused by the check on the device: invalid data, named by its first point; never an out-of-range read
@pytest.mark.parametrize("index", [torch.int32, torch.int64])
def test_refusals_found_on_the_device(pkg, index):
    colptr, rowval, _ = MATRIX
    ext = rowval.size
    wk = pkg.Worker(pkg.PRIOR_MULT, D, N, device=0, seed=3)
    wk.upload_points_csc(colptr, rowval, _values_as(2)[1])
    before = _points(wk)
    nz = _values_as(2)[0].to(DEV)

    def attempt(cp, rv):
        cpd, rvd = torch.from_numpy(cp).to(index).to(DEV), torch.from_numpy(rv).to(index).to(DEV)
        torch.cuda.synchronize()
        wk.upload_points_csc_device(cpd.data_ptr(), _IDX[index], rvd.data_ptr(), nz.data_ptr(), 2, ext, 0)

    def col(i):        # a column with at least three entries at or behind i
        return int(i + np.nonzero(np.diff(colptr)[i:] >= 3)[0][0])

    def with_cp(j, v):
        c = colptr.copy(); c[j] = v
        return c

    def with_rv(i, k, v):
        r = rowval.copy(); r[colptr[i] + k] = v
        return r

    i = col(700)
    sw = rowval.copy(); a = colptr[i]; sw[a + 1], sw[a + 2] = rowval[a + 2], rowval[a + 1]
    j = col(100)                                                     # (inside the run [64, 128) with the bad offset of point j + 1)
    cases = [
        (with_cp(i + 1, colptr[i] - 1), rowval, f"colptr decreases at point {i}"),
        (with_cp(3000, ext + 1), rowval, "colptr points outside rowval / nzval at point 2999"),
        (with_cp(N, ext + 1), rowval, f"colptr points outside rowval / nzval at point {N - 1}"),
        (with_cp(3000, -1), rowval, "colptr points outside rowval / nzval at point 2999"),
        (with_cp(0, -5), rowval, "colptr points outside rowval / nzval at point 0"),
        (colptr, with_rv(i, 1, D), f"point {i}: row index out of range"),
        (colptr, with_rv(i, 0, -1), f"point {i}: row index out of range"),
        (colptr, with_rv(14, D - 1, D + 7), "point 14: row index out of range"),
        (colptr, sw, f"point {i}: row indices are not strictly increasing"),
        (colptr, with_rv(i, 1, rowval[colptr[i]]), f"point {i}: row indices are not strictly increasing"),
        (with_cp(650, ext + 9), with_rv(i, 1, D), "colptr points outside rowval / nzval at point 649"),     # two offenders: the lower point
        (with_cp(i + 1, colptr[i] - 1), with_rv(col(300), 0, D), f"point {col(300)}: row index out of range"),
        (with_cp(j + 2, -1), with_rv(j, 2, -3), f"point {j}: row index out of range"),
    ]
    for cp, rv, what in cases:
        with pytest.raises(pkg.DpmmError, match="dpmm_upload_points_csc_device: " + what.replace("(", r"\(")) as ei:
            attempt(cp, rv)
        assert ei.value.code == -1, what
        assert np.array_equal(_points(wk), before), what
    attempt(colptr * 0, rowval)                                      # the next valid upload succeeds: all points empty ...
    assert not _points(wk).any()
    attempt(colptr, rowval)                                          # ... and the matrix itself
    assert np.array_equal(_points(wk), before)
    wk.close()


# ---- 10. whole chains from a sparse_csc tensor on the GPU
def test_whole_chains_from_a_gpu_csc_tensor(pkg, host, tmp_path):
    Dc, Nc = 200, 6000
    data, y = _topics(Dc, 4, Nc, 40, seed=2)
    cp, rv, nz, shape = data
    csr = torch.sparse_csr_tensor(torch.from_numpy(np.asarray(cp, np.int64)), torch.from_numpy(np.asarray(rv, np.int64)),
                                  torch.from_numpy(np.asarray(nz)).to(torch.int16), size=(Nc, Dc)).to(DEV)      # a bag-of-words matrix, (N, D)
    t = csr.t()
    hyper = host.multinomial_hyper(np.ones(Dc, np.float32))
    kw = dict(iters=30, seed=5, burnout=5, verbose=False)
    ref = host.fit(data, hyper, 10.0, **kw)
    got = host.fit(t, hyper, 10.0, save_model=True, save_path=str(tmp_path) + "/", model_save_interval=15, **kw)
    for a, b in ((ref[0], got[0]), (ref[7], got[7])):
        assert isinstance(b, torch.Tensor) and b.dtype == torch.int64 and b.device == t.device and np.array_equal(a, b.cpu().numpy())
    assert ref[6] == got[6] and max(ref[6]) > 1
    with pytest.raises(TypeError, match="Multinomial"):
        host.fit(t, 10.0, iters=1, verbose=False)
    # predictions.  capacity 1000: six full slabs, every one read in place; capacity 900: six full slabs and a short one of 600 points,
    # which goes through the kept device staging colptr and the staged outputs
    want = host.predict(ref[8], data)
    have = host.predict(got[8], t)
    score = importlib.import_module(pkg.__name__ + ".host.score")
    for cap in (1000, 900):
        assert (Nc % cap != 0) == (cap == 900)
        with score.Predictor(ref[8], capacity=cap) as p:
            want += p.predict_topk(data, 2) + (p.score_samples(data),) + p.predict(data)
            have += p.predict_topk(t, 2) + (p.score_samples(t),) + p.predict(t)
            if cap == 900:
                assert p._csc_stage is not None and p._csc_stage.numel() == cap + 1 and p._csc_stage.device == t.device
                have += p.predict(t)                                  # the staging vector is reused by the next call
                want += p.predict(data)
    for a, b in zip(want, have):
        assert isinstance(b, torch.Tensor) and b.device == t.device
        assert np.array_equal(a.view(np.uint8), b.cpu().numpy().view(np.uint8))
    # a checkpoint of the tensor's chain, resumed with the tensor
    res, *_ = host.resume_from_checkpoint(got[8].checkpoints[0], t, 30, verbose=False)
    assert isinstance(res.labels, torch.Tensor) and torch.equal(res.labels, got[0]) and torch.equal(res.labels_subcluster, got[7])


# ---- 11. LDS and registers poisoned (tests/test_gpu_uninit.py's method): the three new kernels read nothing they did not write
@pytest.mark.parametrize("pattern", [0xffffffff, 0x7fc00000])
def test_the_ingest_kernels_ignore_lds_and_register_contents(pkg, binding, pattern):
    import contextlib
    from tools import poison
    poison.build()                                                    # (a build failure is a failure here, not a skip)
    cp, rv, nz = _device_arrays(torch.int32, 1, _values_as(3)[0])
    want = _host_reference(pkg, 3)
    for dirty in (False, True, "kernels"):
        with (poison.poisoned_kernel_launches(binding, pattern) if dirty == "kernels" else contextlib.nullcontext()):
            wk = pkg.Worker(pkg.PRIOR_MULT, D, N, device=0, seed=3)
            if dirty: poison.poison(pattern)
            wk.upload_points_csc_device(cp.data_ptr(), 6, rv.data_ptr(), nz.data_ptr(), 3, rv.numel(), 1)
            got = _state(wk)
            wk.close()
        _assert_same(got, want)
