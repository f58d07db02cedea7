"""GPU tests of include/dpmm_hip_tensor.h (csrc/tensor_io.hip) and of device tensors through the public entry points.  Every tensor is
built with torch on the device.  Everything is compared bit for bit -- a conversion to Float32 has one right answer (`ref_ingest`,
tests/test_tensor_input_cpu.py, checked there against `tensor.float()`) -- except the one comparison across shards, which is held to the
rtol 1e-12 of test_suffstats_vs_oracle because the association of the Float64 sums differs across shards."""
import importlib

import numpy as np
import pytest
import torch

from test_gpu_mult import make_problem as make_mult
from test_gpu_niw import make_problem as make_niw
from test_tensor_input_cpu import DTYPES, ref_ingest, same_bits, special_values, storage_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INT_CODES = (4, 5, 6, 7)


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def host(pkg):
    return importlib.import_module("dpmmsubclusters_jl_amd.host")


@pytest.fixture(scope="module")
def T(host):
    return importlib.import_module("dpmmsubclusters_jl_amd.host.tensors")


def ldx_of(D):
    return (D + 3) // 4 * 4


def readback(wk, ld_out=None):
    """The points in force as an (n, ld_out) float32 numpy array, through dpmm_get_points_device."""
    ld = ldx_of(wk.D) if ld_out is None else ld_out
    out = torch.full((max(wk.n, 1), ld), -7.0, dtype=torch.float32, device=DEV)[:wk.n]
    torch.cuda.synchronize()
    wk.get_points_device(out.data_ptr(), ld)
    return out.cpu().numpy()


LAYOUTS = ("pm_contiguous", "pm_padded", "pm_padded_odd", "fm_contiguous", "fm_columns_odd_lo", "general", "stride0_points", "stride0_features")


def make_view(code, layout, D, n, seed):
    """A (D, n) view of a device tensor of DTYPES[code] in the named layout, filled with special_values."""
    dt = DTYPES[code]

    def fill(*shape):
        return special_values(dt, int(np.prod(shape)), seed=seed).reshape(*shape).to(DEV)
    if layout == "pm_contiguous":                      # an (N, D) tensor's .T
        return fill(n, D).T
    if layout == "pm_padded":                          # stride_point > D, rows still vector aligned where D % 4 == 0
        return fill(n, D + 8)[:, :D].T
    if layout == "pm_padded_odd":                      # stride_point > D and odd: no vector alignment
        return fill(n, D + 5)[:, 1:1 + D].T
    if layout == "fm_contiguous":
        return fill(D, n)
    if layout == "fm_columns_odd_lo":                  # a column range [lo, hi) with lo = 3
        return fill(D, n + 7)[:, 3:3 + n]
    if layout == "general":
        return fill(2 * D, 3 * n + 1)[::2, ::3][:, :n]
    if layout == "stride0_points":                     # one point, expanded: stride_point = 0
        return fill(D, 1).expand(D, n)
    if layout == "stride0_features":                   # one feature row, expanded: stride_feature = 0
        return fill(1, max(n, 1))[:, :n].expand(D, n)
    raise AssertionError(layout)


def upload_view(wk, T, v, nan_to_zero=False):
    desc = T.describe(v)
    torch.cuda.synchronize()
    wk.upload_points_strided_device(desc.shard_ptr(0), desc.dtype, desc.stride_point, desc.stride_feature, nan_to_zero)
    return desc


def want_of(v, code, n, D, nan_to_zero=False):
    st, off = storage_of(v)
    return ref_ingest(st, code, (v.stride(1), v.stride(0)), n, D, offset=off, nan_to_zero=nan_to_zero)


def byte_path_image(want, D):
    """What a Multinomial context holds for the Float32 image `want`: when EVERY element is an integer in [0, 255] the context keeps a byte
    copy and frees the Float32 matrix (finish_upload, dpmm_api.cpp; u8_convert_kernel, mult_sweep.hip) -- a byte has no sign, so a -0 of
    such an image reads back as +0; every other image is kept as it is.  (A rule of the storage, stated from its source, not from a run.)"""
    v = want[:, :D]
    with np.errstate(invalid="ignore"):
        counts = v.size > 0 and bool(np.all((v >= 0) & (v <= 255) & (np.trunc(v) == v)))
    return np.where(want == 0, np.float32(0), want) if counts else want


NS = (0, 1, 63, 64, 65, 4097)


@pytest.mark.parametrize("D", [1, 2, 5, 63, 64, 100, 256])
def test_ingest_equals_reference_niw(pkg, T, D):
    checked = 0
    for n in NS:
        wk = pkg.Worker(pkg.PRIOR_NIW, D, n, device=0, seed=1)
        for code in range(8):
            for layout in LAYOUTS:
                v = make_view(code, layout, D, n, seed=7 * code + n)
                assert tuple(v.shape) == (D, n)
                upload_view(wk, T, v)
                got = readback(wk)
                assert got.shape == (n, ldx_of(D))
                assert same_bits(got, want_of(v, code, n, D)), (D, n, DTYPES[code], layout)
                assert not got[:, D:].any()
                checked += 1
        wk.close()
    assert checked == len(NS) * 8 * len(LAYOUTS)


@pytest.mark.parametrize("D", [1, 2, 5, 63, 64, 100, 256, 1000])
def test_ingest_equals_reference_multinomial(pkg, T, D):
    """Integer element types and Float32 into Multinomial contexts: the image a Multinomial context derives its byte / bf16 paths from."""
    for n in NS:
        wk = pkg.Worker(pkg.PRIOR_MULT, D, n, device=0, seed=1)
        for code in INT_CODES + (2,):
            for layout in LAYOUTS:
                v = make_view(code, layout, D, n, seed=3 * code + n)
                upload_view(wk, T, v)
                got = readback(wk)
                assert same_bits(got, byte_path_image(want_of(v, code, n, D), D)), (D, n, DTYPES[code], layout)
        wk.close()


def test_nan_to_zero_and_wide_readback(pkg, T):
    D, n = 37, 300
    wk = pkg.Worker(pkg.PRIOR_NIW, D, n, device=0, seed=1)
    for code in (0, 1, 2, 3):
        for layout in ("pm_contiguous", "fm_contiguous", "general"):
            v = make_view(code, layout, D, n, seed=code)
            assert layout == "general" or torch.isnan(v.float()).any()
            upload_view(wk, T, v, nan_to_zero=True)
            got = readback(wk, ld_out=D + 6)                    # an output row wider than ldx, not a multiple of four
            want = want_of(v, code, n, D, nan_to_zero=True)
            assert not np.isnan(got).any() and same_bits(got[:, :D], want[:, :D]) and not got[:, D:].any()
    wk.close()


@pytest.mark.parametrize("code", [2, 1])
def test_headline_points_per_launch(pkg, code):
    """n = 10^6, D = 64 in both main modes: the grid-stride loops and the Int64 index arithmetic run (the reference here is torch's own
    conversion on the device, which test_tensor_input_cpu.py ties to ref_ingest)."""
    n, D = 10 ** 6, 64
    g = torch.Generator(device=DEV).manual_seed(5)
    base = torch.randn(n, D, generator=g, device=DEV).to(DTYPES[code])
    want = base.float().contiguous()
    wk = pkg.Worker(pkg.PRIOR_NIW, D, n, device=0, seed=1)
    out = torch.empty((n, D), dtype=torch.float32, device=DEV)
    for name, v in (("point-major", base.T), ("feature-major", base.T.contiguous())):
        assert tuple(v.shape) == (D, n)
        torch.cuda.synchronize()
        wk.upload_points_strided_device(v.data_ptr(), code, v.stride(1), v.stride(0))
        out.fill_(-1.0)
        torch.cuda.synchronize()
        wk.get_points_device(out.data_ptr(), D)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), name
    wk.close()


# ---------------------------------------------------------------------------------------------- the read-back itself
def test_readback_of_every_point_storage(pkg):
    rng = np.random.default_rng(2)
    # dense NIW after the existing host upload
    for D, n in ((5, 777), (64, 1000), (130, 333)):
        X = rng.standard_normal((n, D)).astype(np.float32)
        wk = pkg.Worker(pkg.PRIOR_NIW, D, n, device=0, seed=1)
        wk.upload_points(X)
        got = readback(wk)
        assert same_bits(got[:, :D], X) and not got[:, D:].any()
        assert same_bits(readback(wk, ld_out=D + 1)[:, :D], X)
        wk.close()
    # Multinomial counts: integers in [0, 255], the byte path (the Float32 matrix is freed); then non-counts: the Float32 matrix again
    D, n = 100, 1500
    C = rng.poisson(3.0, size=(n, D)).astype(np.float32)
    C[5, 7] = 255.0
    wk = pkg.Worker(pkg.PRIOR_MULT, D, n, device=0, seed=1)
    wk.upload_points(C)
    got = readback(wk, ld_out=D + 3)
    assert same_bits(got[:, :D], C) and not got[:, D:].any()
    F = C + np.float32(0.25)
    wk.upload_points(F)
    assert same_bits(readback(wk)[:, :D], F)
    # sparse columns
    C[::4] = 0.0
    r, c = np.nonzero(C)
    colptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=colptr[1:])
    wk.upload_points_csc(colptr, c.astype(np.int64), C[r, c].astype(np.float32))
    got = readback(wk, ld_out=D + 2)
    assert same_bits(got[:, :D], C) and not got[:, D:].any()
    # and back to dense from a device tensor: the sparse points are replaced
    t = torch.from_numpy(np.ascontiguousarray(F)).to(DEV)
    torch.cuda.synchronize()
    wk.upload_points_strided_device(t.data_ptr(), 2, D, 1)
    assert same_bits(readback(wk)[:, :D], F)
    wk.close()


def test_labels_in_and_out_of_device_memory(pkg):
    n, K = 5001, 7
    rng = np.random.default_rng(3)
    lab = rng.integers(1, K + 1, n); sub = rng.integers(1, 3, n)
    wk = pkg.Worker(pkg.PRIOR_NIW, 4, n, device=0, seed=1)
    wk.upload_points(rng.standard_normal((n, 4)).astype(np.float32))
    with pytest.raises(pkg.DpmmError) as e:
        wk.get_labels_tensor(DEV)
    assert e.value.code == -4                                    # DPMM_ESTATE: no labels yet
    tl, ts = torch.from_numpy(lab).to(DEV), torch.from_numpy(sub).to(DEV)
    torch.cuda.synchronize()
    wk.set_labels_device(tl.data_ptr(), ts.data_ptr())
    hl, hs = wk.get_labels()
    assert np.array_equal(hl, lab) and np.array_equal(hs, sub)
    gl, gs = wk.get_labels_tensor(DEV)
    assert gl.dtype == torch.int64 and gl.device == tl.device and torch.equal(gl, tl) and torch.equal(gs, ts)
    only = torch.zeros(n, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    wk.get_labels_device(0, only.data_ptr())                     # either may be NULL
    assert torch.equal(only, ts)
    flipped = 3 - ts
    torch.cuda.synchronize()
    wk.set_labels_device(0, flipped.data_ptr())                  # sub-labels alone
    assert np.array_equal(wk.get_labels()[1], 3 - sub) and np.array_equal(wk.get_labels()[0], lab)
    wk.close()


# ---------------------------------------------------------------------------------------------- same points, same everything
def _main_mode_views(X, dtype=torch.float32):
    """The (n, D) host rows as (D, n) device views in the two main modes."""
    t = torch.from_numpy(np.ascontiguousarray(X)).to(dtype).to(DEV)
    return dict(point_major=t.T, feature_major=t.T.contiguous())


@pytest.mark.parametrize("prior", ["niw", "mult"])
def test_same_points_same_statistics_and_table(pkg, T, prior):
    if prior == "niw":
        P = make_niw(64, 6000, 4, seed=2)
    else:
        P = make_mult(100, 5000, 5, 60, seed=2)
    n, D, K = P["n"], P["D"], P["K"]
    rng = np.random.default_rng(1)
    lab = rng.integers(1, K + 1, n); sub = rng.integers(1, 3, n)

    def run(upload):
        wk = pkg.Worker(pkg.PRIOR_NIW if prior == "niw" else pkg.PRIOR_MULT, D, n, device=0, seed=4)
        upload(wk)
        if prior == "niw":
            wk.set_params_niw(P["mu"], P["invS"], P["logdet"], P["lr"], P["w"])
        else:
            wk.set_params_mult(P["logp"], P["lr"], P["w"])
        wk.set_labels(lab, sub)
        out = (wk.suffstats_packed(), wk.debug_loglik(), readback(wk))
        wk.close()
        return out
    ref = run(lambda wk: wk.upload_points(P["X"]))
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    views = _main_mode_views(P["X"])
    if prior == "mult":
        views["point_major_u8"] = _main_mode_views(P["X"], torch.uint8)["point_major"]
        views["feature_major_i64"] = _main_mode_views(P["X"], torch.int64)["feature_major"]
    for name, v in views.items():
        got = run(lambda wk: upload_view(wk, T, v))
        for a, b in zip(ref, got):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), name


# ---------------------------------------------------------------------------------------------- end to end
def _same_fit(a, b, dev_result):
    """9-tuples of fit: b from the host array, a from the device tensor."""
    assert isinstance(b[0], np.ndarray) and isinstance(b[7], np.ndarray)
    if dev_result:
        for t in (a[0], a[7], a[8].labels, a[8].labels_subcluster):
            assert isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.device == torch.device(DEV)
        assert torch.equal(a[0], a[8].labels) and torch.equal(a[7], a[8].labels_subcluster)
    assert np.array_equal(a[0].cpu().numpy(), b[0]) and np.array_equal(a[7].cpu().numpy(), b[7])
    assert list(a[6]) == list(b[6]) and len(a[3]) == len(b[3])            # (iter_count holds the iterations' wall times)
    assert np.array_equal(np.asarray(a[2]), np.asarray(b[2]))
    assert np.array_equal(np.asarray(a[5]), np.asarray(b[5]))


def test_fit_from_device_tensors_is_the_host_chain(host):
    """fit(x_dev) = fit(x_dev.float().cpu().numpy()) with the same seed: labels, sub-labels, cluster-count history, weights, likelihoods."""
    # the docs example (config C1), Float32, contiguous (D, N)
    x, y, _, _ = host.generate_gaussian_data(10 ** 4, 2, 6, 100.0, seed=4)
    xd = torch.from_numpy(x).to(DEV)
    kw = dict(iters=100, burnout=10, seed=12345, verbose=False)
    a = host.fit(xd, 10.0, gt=torch.from_numpy(y).to(DEV), **kw)
    b = host.fit(xd.float().cpu().numpy(), 10.0, gt=y, **kw)
    _same_fit(a, b, True)
    assert a[4] == b[4] and a[4][-1] > 0.9 and b[6][-1] >= 5
    # D = 64: an (N, D) bfloat16 tensor of embeddings passed as .T, and Float16 / Float64 feature-major
    x, y, _, _ = host.generate_gaussian_data(30000, 64, 6, 100.0, seed=3)
    emb = torch.from_numpy(np.ascontiguousarray(x.T)).to(DEV)
    kw = dict(iters=40, burnout=8, seed=7, verbose=False)
    for name, xd in dict(bf16_T=emb.to(torch.bfloat16).T, f32_T=emb.T, f16_fm=emb.T.contiguous().to(torch.float16),
                         f64_cols=torch.from_numpy(x.astype(np.float64)).to(DEV)[:, 5:20005]).items():
        assert xd.shape[0] == 64
        a = host.fit(xd, 10.0, **kw)
        b = host.fit(xd.float().cpu().numpy(), 10.0, **kw)
        _same_fit(a, b, True)
        assert b[6][-1] >= 3, name
    # Multinomial D = 100: counts as int32 (N, D).T and uint8 (D, N)
    x, _, _ = host.generate_mnmm_data(20000, 100, 5, 80, seed=6)
    hyper = host.multinomial_hyper(np.ones(100))
    kw = dict(iters=40, burnout=5, seed=11, verbose=False)
    b = host.fit(x, hyper, 10.0, **kw)
    assert b[6][-1] >= 3
    for xd in (torch.from_numpy(np.ascontiguousarray(x.T)).to(torch.int32).to(DEV).T, torch.from_numpy(x).to(torch.uint8).to(DEV)):
        a = host.fit(xd, hyper, 10.0, **kw)
        _same_fit(a, b, True)
    # a disagreeing device is refused
    with pytest.raises(ValueError, match="disagrees"):
        host.fit(xd, hyper, 10.0, device=1, **kw)


def test_predict_from_a_device_tensor(host):
    x, y, _, _ = host.generate_gaussian_data(20000, 8, 5, 80.0, seed=2)
    res = host.fit(x, 10.0, iters=40, burnout=8, seed=3, verbose=False)
    model = res[8]
    q = torch.from_numpy(np.ascontiguousarray(x[:, :7001].T)).to(torch.bfloat16).to(DEV)      # (n, D) embeddings
    la, pa = host.predict(model, q.T)
    lb, pb = host.predict(model, q.T.float().cpu().numpy())
    assert isinstance(la, torch.Tensor) and isinstance(pa, torch.Tensor) and la.device == q.device and pa.device == q.device
    assert la.dtype == torch.int64 and pa.dtype == torch.float32 and tuple(pa.shape) == (7001, model.num_clusters)
    assert isinstance(lb, np.ndarray) and isinstance(pb, np.ndarray)
    assert np.array_equal(la.cpu().numpy(), lb) and pa.cpu().numpy().tobytes() == pb.tobytes()
    assert model.num_clusters >= 3 and np.isfinite(pb).all()
    # Multinomial, feature-major counts
    x, _, _ = host.generate_mnmm_data(6000, 50, 4, 60, seed=3)
    res = host.fit(x, host.multinomial_hyper(np.ones(50)), 10.0, iters=30, burnout=5, seed=2, verbose=False)
    la, pa = host.predict(res[8], torch.from_numpy(x).to(torch.int16).to(DEV))
    lb, pb = host.predict(res[8], x)
    assert np.array_equal(la.cpu().numpy(), lb) and pa.cpu().numpy().tobytes() == pb.tobytes()


def test_resume_from_checkpoint_with_a_device_tensor(host, tmp_path):
    x, y = host.generate_gaussian_data(3000, 3, 3, 60.0, seed=4)[:2]
    x = x.astype(np.float32)
    xd = torch.from_numpy(np.ascontiguousarray(x.T)).to(DEV).T
    r = host.fit(xd, 10.0, iters=10, seed=5, burnout=4, verbose=False, save_model=True, save_path=str(tmp_path) + "/", model_save_interval=5)
    model = r[8]
    assert len(model.checkpoints) == 2
    res_d, *_ = host.resume_from_checkpoint(model.checkpoints[0], xd, 10, verbose=False)
    res_h, *_ = host.resume_from_checkpoint(model.checkpoints[0], x, 10, verbose=False)
    assert isinstance(res_d.labels, torch.Tensor) and res_d.labels.device == xd.device and isinstance(res_h.labels, np.ndarray)
    assert torch.equal(res_d.labels, r[0]) and np.array_equal(res_h.labels, r[0].cpu().numpy())
    assert np.array_equal(res_d.labels_subcluster.cpu().numpy(), res_h.labels_subcluster)
    assert res_d.sampler.K == res_h.sampler.K == model.sampler.K and np.array_equal(res_d.sampler.weights, res_h.sampler.weights)


# ---------------------------------------------------------------------------------------------- shards
@pytest.mark.parametrize("layout", ["pm_contiguous", "fm_contiguous", "fm_columns_odd_lo", "general"])
def test_two_shards_of_one_tensor(pkg, T, layout):
    """Two workers ingest [0, lo) and [lo, N) of ONE device tensor through the description's offset arithmetic (N and lo odd)."""
    D, N, K, lo = 64, 9001, 5, 4501
    rng = np.random.default_rng(4)
    if layout == "pm_contiguous":
        v = torch.from_numpy(rng.standard_normal((N, D)).astype(np.float32)).to(DEV).T
    elif layout == "fm_contiguous":
        v = torch.from_numpy(rng.standard_normal((D, N)).astype(np.float32)).to(DEV)
    elif layout == "fm_columns_odd_lo":
        v = torch.from_numpy(rng.standard_normal((D, N + 7)).astype(np.float32)).to(DEV)[:, 3:3 + N]
    else:
        v = torch.from_numpy(rng.standard_normal((2 * D, 3 * N + 1)).astype(np.float32)).to(DEV)[::2, ::3][:, :N]
    assert tuple(v.shape) == (D, N)
    desc = T.describe(v)
    lab = rng.integers(1, K + 1, N); sub = rng.integers(1, 3, N)
    rows, images = [], []
    for first, a, b in ((0, 0, N), (0, 0, lo), (lo, lo, N)):
        wk = pkg.Worker(pkg.PRIOR_NIW, D, b - a, first_index=first, device=0, seed=4)
        torch.cuda.synchronize()
        wk.upload_points_tensor(desc, a, b)
        wk.set_labels(lab[a:b], sub[a:b])
        wk.set_params_niw_chol(np.zeros((3 * K, D)), np.tile(np.eye(D).ravel(), (3 * K, 1)), np.zeros(3 * K), np.full((K, 2), 0.5), np.full(K, 1.0 / K))
        rows.append(wk.suffstats_packed())
        images.append(readback(wk))
        wk.close()
    whole = v.float().cpu().numpy().T
    assert same_bits(images[0], whole) and same_bits(np.concatenate(images[1:]), whole)
    wk = pkg.Worker(pkg.PRIOR_NIW, D, 1, device=0, seed=4)        # (unpacking is a host-side function of the context's layout)
    (N1, s1, S1), (N2, s2, S2) = wk.unpack(rows[0], K), wk.unpack(rows[1] + rows[2], K)
    wk.close()
    assert np.array_equal(N1, N2) and N1[:, 0].sum() == N          # the counts: exact
    np.testing.assert_allclose(s2, s1, rtol=1e-12, atol=1e-10)      # the tolerances of test_suffstats_vs_oracle, no tighter
    np.testing.assert_allclose(S2, S1, rtol=1e-12, atol=1e-9)


# ---------------------------------------------------------------------------------------------- refusals instead of faults
def test_bad_arguments_are_refused_before_any_launch(pkg):
    """Every call below hands the library something it must reject with DPMM_EINVAL BEFORE it launches anything; the points in force stay."""
    D, n = 64, 4097
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, D)).astype(np.float32)
    wk = pkg.Worker(pkg.PRIOR_NIW, D, n, device=0, seed=1)
    wk.upload_points(X)
    good = torch.from_numpy(X).to(DEV)
    small = torch.zeros(16, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()

    def refused(call, *what):
        with pytest.raises(pkg.DpmmError) as e:
            call()
        assert e.value.code == -1, str(e.value)
        for w in what:
            assert w in str(e.value), str(e.value)
        assert same_bits(readback(wk), X)                        # the points in force are untouched

    host_rows = np.ascontiguousarray(X)
    refused(lambda: wk.upload_points_strided_device(host_rows.ctypes.data, 2, D, 1), "d_src")                       # a host pointer
    refused(lambda: wk.upload_points_strided_device(0, 2, D, 1), "d_src", "null")
    refused(lambda: wk.upload_points_strided_device(small.data_ptr(), 2, 1 << 20, 1), "d_src", "allocation")        # 16 GB addressed from 64 bytes
    refused(lambda: wk.upload_points_strided_device(small.data_ptr(), 2, 1, 1 << 24), "d_src", "allocation")
    refused(lambda: wk.upload_points_strided_device(good.data_ptr() + 2, 2, D, 1), "d_src", "aligned")              # misaligned for Float32
    refused(lambda: wk.upload_points_strided_device(good.data_ptr() + 4, 3, D, 1), "d_src", "aligned")              # ... for Float64
    refused(lambda: wk.upload_points_strided_device(good.data_ptr(), 8, D, 1), "dtype")                             # unknown codes
    refused(lambda: wk.upload_points_strided_device(good.data_ptr(), -1, D, 1), "dtype")
    refused(lambda: wk.upload_points_strided_device(good.data_ptr(), 2, -D, 1), "negative")
    refused(lambda: wk.upload_points_strided_device(good.data_ptr(), 2, 1 << 61, 1 << 61))                          # an extent beyond any address space
    refused(lambda: wk.get_points_device(small.data_ptr(), 1 << 16), "d_out", "allocation")                         # 1 GB into 64 bytes
    refused(lambda: wk.get_points_device(host_rows.ctypes.data, D), "d_out")
    refused(lambda: wk.get_points_device(good.data_ptr(), D - 1), "ld_out")
    wk.init_labels(3, 1)
    big_n = pkg.Worker(pkg.PRIOR_NIW, 2, 1 << 24, device=0, seed=1)                                                # 128 MB of labels into 64 bytes
    big_n.init_labels(2, 1)
    for call in (lambda: big_n.get_labels_device(small.data_ptr(), 0), lambda: big_n.set_labels_device(small.data_ptr(), small.data_ptr())):
        with pytest.raises(pkg.DpmmError) as e:
            call()
        assert e.value.code == -1 and "allocation" in str(e.value)
    big_n.close()
    lab = np.empty(n, np.int64)
    refused(lambda: wk.get_labels_device(lab.ctypes.data, 0), "d_labels")
    # the valid call still works afterwards
    wk.upload_points_strided_device(good.data_ptr(), 2, D, 1)
    assert same_bits(readback(wk), X)
    wk.close()


def test_predict_into_too_small_a_buffer_is_refused(pkg):
    D, n, K = 8, 1 << 19, 3
    rng = np.random.default_rng(1)
    X = rng.standard_normal((n, D)).astype(np.float32)
    wk = pkg.Worker(pkg.PRIOR_NIW, D, n, device=0, seed=1)
    wk.upload_points(X)
    R = np.stack([np.eye(D, dtype=np.float32)] * K)
    args = (rng.standard_normal((K, D)).astype(np.float32), R.reshape(K, -1), np.zeros(K, np.float32), np.full(K, 5.0, np.float32),
            np.full(K, 1.0 / K, np.float32))
    host_lab, host_probs = wk.predict_table_niw(*args, points=True)
    small = torch.zeros(16, dtype=torch.int64, device=DEV)
    labels = torch.zeros(n, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    for call, arg in ((lambda: wk.predict_points_device(small.data_ptr(), 0), "d_labels"),                  # 4 MB into 128 bytes
                      (lambda: wk.predict_points_device(labels.data_ptr(), small.data_ptr()), "d_probs")):  # 6 MB into 128 bytes
        with pytest.raises(pkg.DpmmError) as e:
            call()
        assert e.value.code == -1 and arg in str(e.value) and "allocation" in str(e.value)
    wk.predict_points_device(labels.data_ptr(), 0)               # probabilities may be NULL
    assert np.array_equal(labels.cpu().numpy(), host_lab)
    probs = torch.zeros((n, K), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    wk.predict_points_device(labels.data_ptr(), probs.data_ptr())
    assert np.array_equal(labels.cpu().numpy(), host_lab) and probs.cpu().numpy().tobytes() == host_probs.tobytes()
    wk.close()
