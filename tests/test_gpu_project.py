"""include/dpmm_hip_project.h on the GPU: the projected uploads against Float64, over shapes, element types and layouts; shard invariance;
non-finite sources; refusals; and `fit` / `predict` / `Predictor` with `project=` against the same calls on pre-projected coordinates.

The acceptance bound of the values: |y - y64| <= (D_in + 8) 2^-24 sum_d |x_d| |W_dj| + 2^-24 |b_j| with
y64 = x32 W - mu' W in Float64 from the Float32-rounded source -- D_in Float32 accumulations, the dropped plane products, the bias rounding.
A one-plane W misses it by orders of magnitude (2^-9 per product)."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def binding(pkg):
    return importlib.import_module(pkg.__name__ + ".binding")


@pytest.fixture(scope="module")
def host(pkg):
    return importlib.import_module(pkg.__name__ + ".host")


@pytest.fixture(scope="module")
def project(pkg):
    return importlib.import_module(pkg.__name__ + ".host.project")


DEV = "cuda"
TORCH_DT = ("float16", "bfloat16", "float32", "float64", "uint8", "int16", "int32", "int64")


def hip_runtime():
    """The HIP runtime of this process (torch's copy: the one the library resolved its symbols against)."""
    path = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    lib = ctypes.CDLL(path if os.path.exists(path) else "libamdhip64.so")
    lib.hipMalloc.argtypes, lib.hipMalloc.restype = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t], ctypes.c_int
    lib.hipFree.argtypes, lib.hipFree.restype = [ctypes.c_void_p], ctypes.c_int
    return lib


def tile_points(d):
    """Points a workgroup of csrc/project.hip owns (proj_tile_points)."""
    return 512 if d <= 64 else 256 if d <= 128 else 128


def read_points(wk, d):
    out = torch.empty((wk.n, d), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    wk.get_points_device(out.data_ptr(), d)
    return out.cpu().numpy()


def upload_view(binding, wk, view, lo=0):
    """view: (D_in, N) tensor on the GPU, any strides; the worker takes its points lo .. lo + wk.n."""
    code = TORCH_DT.index(str(view.dtype).split(".")[1])
    torch.cuda.synchronize()
    wk.upload_points_projected_strided_device(view.data_ptr() + lo * view.stride(1) * view.element_size(), code, view.stride(1), view.stride(0))


def source(rng, n, D_in, code):
    """(n, D_in) tensor on the GPU of the DT code's type; integer types over their own range."""
    name = TORCH_DT[code]
    if code in (0, 1, 2, 3):
        a = rng.standard_normal((n, D_in)) * np.exp(rng.uniform(-2, 2, (n, D_in)))
        return torch.from_numpy(a).to(DEV).to(getattr(torch, name))
    info = np.iinfo(name)
    a = rng.integers(info.min, info.max, (n, D_in), dtype=name, endpoint=True)
    return torch.from_numpy(a).to(DEV)


def check_values(binding, rng, D_in, d, n, code):
    W = rng.standard_normal((D_in, d)) / np.sqrt(D_in)
    mu = rng.standard_normal(D_in)
    x = source(rng, n, D_in, code)
    wk = binding.Worker(binding.PRIOR_NIW, d, n, timing=False)
    try:
        wk.set_projection(W, mu)
        upload_view(binding, wk, x.T)
        y = read_points(wk, d).astype(np.float64)
    finally:
        wk.close()
    x32 = x.float().cpu().numpy().astype(np.float64)
    b = mu @ W
    y64 = x32 @ W - b
    den = np.abs(x32) @ np.abs(W)
    bound = (D_in + 8) * 2.0 ** -24 * den + 2.0 ** -24 * np.abs(b)
    err = np.abs(y - y64)
    rel = float((err / np.maximum(den, 1e-300)).max())
    print(f"D_in {D_in} d {d} n {n} {TORCH_DT[code]}: max |y - y64| / sum|x||W| = {rel:.3e}  (bound factor {(D_in + 8) * 2.0 ** -24:.3e})")
    assert np.isfinite(y).all()
    assert (err <= bound).all(), (float((err - bound).max()), rel)


SHAPES = [(1, 1), (31, 2), (257, 33), (384, 64), (1000, 200), (4096, 256)]


@pytest.mark.parametrize("D_in,d", SHAPES)
def test_values_against_float64_over_shapes(binding, D_in, d):
    rng = np.random.default_rng(1000 * D_in + d)
    for n in (1, 63, 64, 65, tile_points(d) + 1):
        check_values(binding, rng, D_in, d, n, 2)
        check_values(binding, rng, D_in, d, n, 1)


@pytest.mark.parametrize("code", range(8))
def test_values_against_float64_every_dtype(binding, code):
    check_values(binding, np.random.default_rng(50 + code), 384, 64, 65, code)
    check_values(binding, np.random.default_rng(60 + code), 384, 64, 513, code)


@pytest.mark.parametrize("name", ["bfloat16", "float32"])
def test_layouts_give_the_bits_of_the_host_call(binding, name):
    D_in, d, n = 257, 33, 300
    rng = np.random.default_rng(7)
    dt = getattr(torch, name)
    W, mu = rng.standard_normal((D_in, d)), rng.standard_normal(D_in)
    vals = torch.from_numpy(rng.standard_normal((n, D_in))).to(dt)             # (n, D_in) on the host: THE values
    wk = binding.Worker(binding.PRIOR_NIW, d, n, timing=False)
    try:
        wk.set_projection(W, mu)
        wk.upload_points_projected(vals.float().numpy())
        ref = read_points(wk, d)
        assert np.isfinite(ref).all()
        g = vals.to(DEV)
        views = {"(N, D_in).T": g.T, "contiguous (D_in, N)": g.T.contiguous()}
        big = torch.zeros((2 * n, 3 * D_in), dtype=dt, device=DEV)
        big[::2, ::3] = g
        views["every second point, every third feature"] = big[::2, ::3].T
        odd = torch.zeros((n, D_in + 1), dtype=dt, device=DEV)
        odd[:, 1:] = g
        views["rows that start at an odd element"] = odd[:, 1:].T
        # the wide loads (every row start 16-byte aligned) against the gather's bits; the last lane's eight features straddle D_in
        pad = torch.full((n, 264), float("nan"), dtype=dt, device=DEV)
        pad[:, :D_in] = g
        assert pad.data_ptr() % 16 == 0 and (264 * pad.element_size()) % 16 == 0
        views["wide loads, D_in not a multiple of the load width"] = pad[:, :D_in].T
        for what, v in views.items():
            assert tuple(v.shape) == (D_in, n)
            wk.upload_points(np.zeros((n, d), np.float32))
            upload_view(binding, wk, v)
            assert np.array_equal(read_points(wk, d).view(np.int32), ref.view(np.int32)), what
        # stride 0: one point expanded to n, one feature expanded to D_in
        one = g[5:6].T.expand(D_in, n)
        upload_view(binding, wk, one)
        assert np.array_equal(read_points(wk, d).view(np.int32), np.repeat(ref[5:6], n, 0).view(np.int32))
        col = g[:, 3:4].T.expand(D_in, n)
        upload_view(binding, wk, col)
        wk2 = read_points(wk, d)
        wk.upload_points_projected(np.ascontiguousarray(vals[:, 3:4].float().numpy().repeat(D_in, 1)))
        assert np.array_equal(wk2.view(np.int32), read_points(wk, d).view(np.int32))
    finally:
        wk.close()


def test_a_shard_equals_the_rows_of_the_whole(binding):
    D_in, d, n, lo, hi = 384, 64, 1200, 37, 37 + 600
    rng = np.random.default_rng(9)
    W, mu = rng.standard_normal((D_in, d)), rng.standard_normal(D_in)
    for dt in (torch.bfloat16, torch.float32):
        g = torch.from_numpy(rng.standard_normal((n, D_in))).to(DEV).to(dt)
        whole, part = binding.Worker(binding.PRIOR_NIW, d, n, timing=False), binding.Worker(binding.PRIOR_NIW, d, hi - lo, first_index=lo, timing=False)
        try:
            for wk in (whole, part):
                wk.set_projection(W, mu)
            upload_view(binding, whole, g.T)
            upload_view(binding, part, g.T, lo=lo)
            assert np.array_equal(read_points(part, d).view(np.int32), read_points(whole, d)[lo:hi].view(np.int32))
        finally:
            whole.close(); part.close()


@pytest.mark.parametrize("name", ["bfloat16", "float32", "float16", "float64"])
def test_a_non_finite_feature_makes_the_whole_point_nan(binding, name):
    D_in, d, n = 257, 33, 70
    rng = np.random.default_rng(3)
    W = rng.standard_normal((D_in, d)); W[200] = 0.0                           # a zero row of W must not hide an Inf (no reliance on Inf * 0)
    g = torch.from_numpy(rng.standard_normal((n, D_in))).to(DEV).to(getattr(torch, name))
    wk = binding.Worker(binding.PRIOR_NIW, d, n, timing=False)
    try:
        wk.set_projection(W, None)
        upload_view(binding, wk, g.T)
        clean = read_points(wk, d)
        g[3, 256] = float("nan")
        g[17, 200] = float("inf")
        g[40, 0] = float("inf"); g[40, 100] = float("-inf")
        upload_view(binding, wk, g.T)
        y = read_points(wk, d)
    finally:
        wk.close()
    bad = np.zeros(n, bool); bad[[3, 17, 40]] = True
    assert np.isnan(y[bad]).all()
    assert np.array_equal(y[~bad].view(np.int32), clean[~bad].view(np.int32))  # its neighbours in the tile are untouched


def test_refusals_launch_nothing_and_leave_the_points(binding):
    D_in, d, n = 40, 8, 50
    rng = np.random.default_rng(2)
    W = rng.standard_normal((D_in, d))
    g = torch.from_numpy(rng.standard_normal((n, D_in)).astype(np.float32)).to(DEV)
    keep = rng.standard_normal((n, d)).astype(np.float32)
    wk = binding.Worker(binding.PRIOR_NIW, d, n, timing=False)
    try:
        wk.upload_points(keep)
        with pytest.raises(binding.DpmmError) as e:                             # no projection set
            upload_view(binding, wk, g.T)
        assert e.value.code == -1 and "projection" in str(e.value)
        with pytest.raises(binding.DpmmError) as e:
            wk.upload_points_projected(np.zeros((n, D_in), np.float32))
        assert e.value.code == -1
        with pytest.raises(binding.DpmmError) as e:                             # D_in = 4097
            wk.set_projection(np.zeros((4097, d)), None)
        assert e.value.code == -5
        bad = W.copy(); bad[7, 3] = np.inf
        with pytest.raises(binding.DpmmError) as e:
            wk.set_projection(bad, None)
        assert e.value.code == -1 and "W" in str(e.value)
        with pytest.raises(binding.DpmmError) as e:
            wk.set_projection(W, np.full(D_in, np.nan))
        assert e.value.code == -1 and "mu" in str(e.value)
        wk.set_projection(W, None)
        hostmem = np.zeros((n, D_in), np.float32)
        with pytest.raises(binding.DpmmError) as e:                             # a host pointer
            wk.upload_points_projected_strided_device(hostmem.ctypes.data, binding.DT_F32, D_in, 1)
        assert e.value.code == -1 and "d_src" in str(e.value)
        # one element too short for the stated strides: an allocation of exactly that size (torch's allocator rounds its blocks up)
        hip = hip_runtime()
        short = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(short), ctypes.c_size_t(4 * (n * D_in - 1))) == 0
        try:
            with pytest.raises(binding.DpmmError) as e:
                wk.upload_points_projected_strided_device(short.value, binding.DT_F32, D_in, 1)
            assert e.value.code == -1 and "d_src" in str(e.value) and "allocation" in str(e.value)
            with pytest.raises(binding.DpmmError) as e:                         # ... and with the strides of the transposed layout
                wk.upload_points_projected_strided_device(short.value, binding.DT_F32, 1, n)
            assert e.value.code == -1 and "allocation" in str(e.value)
        finally:
            assert hip.hipFree(short) == 0
        with pytest.raises(binding.DpmmError):
            wk.upload_points_projected_strided_device(g.data_ptr(), 8, D_in, 1)
        with pytest.raises(binding.DpmmError):
            wk.upload_points_projected_strided_device(g.data_ptr(), binding.DT_F32, -1, 1)
        assert np.array_equal(read_points(wk, d), keep)                         # the points in force are the ones from before
        upload_view(binding, wk, g.T)                                           # ... and the projection survived all of it
        y = read_points(wk, d)
        assert np.abs(y - g.cpu().numpy().astype(np.float64) @ W).max() < 1e-3
        wk.upload_points(keep)                                                  # it survives uploads and does not change the points in force
        wk.clear_projection()
        assert np.array_equal(read_points(wk, d), keep)
        with pytest.raises(binding.DpmmError):
            upload_view(binding, wk, g.T)
    finally:
        wk.close()
    mult = binding.Worker(binding.PRIOR_MULT, d, n, timing=False)
    try:
        with pytest.raises(binding.DpmmError) as e:                             # a Multinomial ctx
            mult.set_projection(W, None)
        assert e.value.code == -1
    finally:
        mult.close()


def test_fit_and_predict_with_a_projection_equal_the_pre_projected_run(host, project, tmp_path):
    D_in, n, K, sub = 384, 6000, 6, 8
    rng = np.random.default_rng(21)
    basis = np.linalg.qr(rng.standard_normal((D_in, sub)))[0]
    centres = rng.standard_normal((K, sub)) * 12
    z = rng.integers(0, K, n)
    X = ((centres[z] + rng.standard_normal((n, sub))) @ basis.T + 0.01 * rng.standard_normal((n, D_in)))
    emb = torch.from_numpy(X).to(DEV).to(torch.bfloat16)                        # (n, D_in): embeddings as a user holds them
    P = project.fit_projection(emb.T, sub, sample=2000, seed=1)
    Y = P.transform(emb.T, capacity=2500)
    assert tuple(Y.shape) == (sub, n) and Y.dtype == torch.float32 and Y.stride() == (1, sub) and Y.device == emb.device
    kw = dict(iters=30, seed=5, verbose=False)
    a = host.fit(emb.T, 10.0, project=P, **kw)
    b = host.fit(Y, 10.0, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[7], b[7])
    ma, mb = a[-1], b[-1]
    assert ma.projection is P and mb.projection is None and ma.sampler.prior.dim == sub
    found = len(np.unique(a[0].cpu().numpy()))
    print("clusters found:", found)
    la, pa = host.predict(ma, emb.T)
    lb, pb = host.predict(ma, Y)
    assert torch.equal(la, lb) and torch.equal(pa.view(torch.int32), pb.view(torch.int32))
    with host.Predictor(ma, capacity=1000) as p:
        for r, s in zip(p.predict(emb.T), (la, pa)):
            assert torch.equal(r, s)
        assert torch.equal(p.score_samples(emb.T).view(torch.int32), p.score_samples(Y).view(torch.int32))
        path = str(tmp_path / "model.npz")
        p.save(path)
    with host.Predictor(ma, capacity=1100) as p:                                # a short last slab: the Float32 staging, projected
        for r, s in zip(p.predict(emb.T), (la, pa)):
            assert torch.equal(r, s)
        lh, ph = p.predict(emb.T.float().cpu().numpy())                         # ... and the same points from the host: the host staging, D_in wide
        assert np.array_equal(lh, la.cpu().numpy()) and np.array_equal(ph.view(np.int32), pa.cpu().numpy().view(np.int32))
        assert p._host_stage_in.shape == (1100, D_in) and p._dev_stage_in.shape == (1100, D_in)
    with host.Predictor.load(path, capacity=1000) as q:
        assert q.projection is not None and q.projection.basis.tobytes() == P.basis.tobytes()
        for r, s in zip(q.predict(emb.T), (la, pa)):
            assert torch.equal(r, s)
    c = host.fit(emb.T, 10.0, project=8, iters=5, seed=5, verbose=False)
    assert c[-1].projection.d == 8 and c[-1].projection.D_in == D_in
