"""GPU tests of include/dpmm_hip_overlap.h (csrc/overlap.hip) and of host/score.py's Predictor.overlap.

The reference is numpy Float64 on the probabilities `predict` returns for the same data (tests/tools/overlap_ref.from_probs): the
matrix P.T @ P, the column sums, np.bincount of the labels over the points that take part.  Two Float64 summations of n non-negative
terms agree within a relative n * 2^-52 -- the header's bound and the tolerance of every comparison of `matrix` and `mass`; `count` and
`skipped` are compared exactly, the symmetry bit for bit.  Models are written to .npz without a fit (write_model of
tests/test_gpu_rank.py) and opened with Predictor.load.  Shapes: K across the 16-row tiles and the 64-row blocks (1, 5, 16, 17, 70, and
1024: every pair of row blocks), n across the 64-point batch and the 256-point tile (1, 256, 261)."""
import importlib

import numpy as np
import pytest
import torch

import test_gpu_rank as G
import test_gpu_score as S
from tools import overlap_ref, rank_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def binding(pkg):
    return importlib.import_module(pkg.__name__ + ".binding")


@pytest.fixture(scope="module")
def host(pkg):
    return importlib.import_module(pkg.__name__ + ".host")


@pytest.fixture(scope="module", autouse=True)
def _close_workers():
    yield
    for wk, _ in G._cache.values():
        wk.close()
    G._cache.clear()


def as_np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def same(a, b):
    """Equal shapes, types and bits."""
    a, b = np.ascontiguousarray(as_np(a)), np.ascontiguousarray(as_np(b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def as_dict(ov):
    return dict(overlap=ov.matrix, mass=ov.mass, count=ov.count, skipped=ov.skipped)


def check(got, want, n, what=""):
    """got, want: dicts overlap / mass / count / skipped; n: the points accumulated.  The bound, exact integers, symmetry, the invariants."""
    O, mass = np.asarray(got["overlap"]), np.asarray(got["mass"])
    K = mass.size
    skipped = int(np.asarray(got["skipped"]).reshape(-1)[0])
    assert O.dtype == np.float64 and mass.dtype == np.float64 and np.asarray(got["count"]).dtype == np.int64
    dO = np.abs(O - want["overlap"]) / np.maximum(np.maximum(O, want["overlap"]), 1e-300)
    dm = np.abs(mass - want["mass"]) / np.maximum(np.maximum(mass, want["mass"]), 1e-300)
    print(what, "K", K, "n", n, "max rel. difference in units of n 2^-52: matrix", dO.max() / overlap_ref.bound(n), "mass", dm.max() / overlap_ref.bound(n))
    assert np.array_equal(np.asarray(got["count"]), want["count"]), what
    assert skipped == int(np.asarray(want["skipped"]).reshape(-1)[0]), what
    assert overlap_ref.close(O, want["overlap"], n), (what, dO.max())
    assert overlap_ref.close(mass, want["mass"], n), (what, dm.max())
    assert np.array_equal(O.view(np.uint64), O.T.copy().view(np.uint64)), what                     # symmetric bit for bit
    assert np.all(np.abs(O.sum(1) - mass) <= mass * (K * 2.0 ** -24 + n * 2.0 ** -52)), what       # rows of probabilities sum to 1
    assert abs(mass.sum() - (n - skipped)) <= n * K * 2.0 ** -24, what
    assert int(np.asarray(got["count"]).sum()) + skipped == n, what


def reference(p, X):
    """What the definitions make of `predict`'s output for the same data, same Predictor."""
    lab, P = p.predict(X)
    return overlap_ref.from_probs(as_np(P), as_np(lab))


def niw_data(post, n, rng, spread=1.5):
    K, D = post["post_m"].shape
    return (post["post_m"][rng.integers(0, K, n)] + spread * rng.standard_normal((n, D))).T.astype(np.float32)      # (D, n)


def run(wk, n_valid=None):
    wk.overlap_begin()
    wk.overlap_accumulate(wk.n if n_valid is None else n_valid)
    return wk.overlap_read()


def worker_reference(wk, tab, n_valid=None):
    """From the worker's own probabilities (dpmm_predict_points) and table: who takes part is read off the table."""
    lab, P = wk._predict_points(wk.K)
    nv = wk.n if n_valid is None else n_valid
    _, _, part = rank_ref.labels_and_scores(tab[:, :nv])
    return overlap_ref.from_probs(P[:nv], lab[:nv], part)


# ------------------------------------------------------------------------------------------------ K and n across the tile edges
@pytest.mark.parametrize("K", [1, 5, 16, 17, 70])
def test_edges_of_K_and_n(host, tmp_path, K):
    rng = np.random.default_rng(100 + K)
    path = str(tmp_path / "m.npz")
    post = G.write_model(path, "niw", 8, K, rng)
    for n in (1, 256, 261):
        X = niw_data(post, n, rng)
        with host.Predictor.load(path, capacity=n) as p:
            got = p.overlap(X)
            want = reference(p, X)
        assert isinstance(got, host.Overlap) and isinstance(got.matrix, np.ndarray) and got.matrix.shape == (K, K) and got.skipped == 0
        check(as_dict(got), want, n, ("edges", K, n))


def test_every_pair_of_row_blocks_at_K_1024(host, tmp_path):
    K, D, n = 1024, 4, 261
    rng = np.random.default_rng(1024)
    path = str(tmp_path / "m.npz")
    post = G.write_model(path, "niw", D, K, rng)
    X = niw_data(post, n, rng, spread=3.0)
    with host.Predictor.load(path, capacity=n) as p:
        got = p.overlap(X)
        want = reference(p, X)
    check(as_dict(got), want, n, "K = 1024")
    assert (got.matrix[960:, :64] > 0).any() and (got.matrix[1023] > 0).any()                     # the last block pair and the last row are filled


# ------------------------------------------------------------------------------------------------ storage paths
@pytest.mark.parametrize("name", ["niw2", "niw64", "mult_u8", "mult_sparse"])
def test_every_storage_path_and_the_table_budget(pkg, binding, name):
    wk, tab = G.cached(pkg, name)
    n = wk.n
    want = worker_reference(wk, tab)
    assert want["skipped"] == 0
    whole = run(wk)
    check(whole, want, n, name)
    kind, D = S.PATHS[name]
    rows = G.K0 * (1 if kind == "niw" else 3)
    try:
        for mb in (0.0, 2 * rows * S.tile_of(kind, D) * 4 / 2.0 ** 20):      # one-tile ranges | two-tile ranges: the last is one tile + 5 points
            wk.set_option(binding.OPT_SCORE_TABLE_MB, mb)
            got = run(wk)
            check(got, want, n, (name, mb))
            assert overlap_ref.close(got["overlap"], whole["overlap"], n) and overlap_ref.close(got["mass"], whole["mass"], n)
            assert np.array_equal(got["count"], whole["count"]) and np.array_equal(got["skipped"], whole["skipped"])
    finally:
        wk.set_option(binding.OPT_SCORE_TABLE_MB, -1)


def test_host_arrays_and_device_tensors_give_equal_bits(host, tmp_path):
    import scipy.sparse as sp
    rng = np.random.default_rng(33)
    n = 2 * 256 + 5
    path = str(tmp_path / "niw.npz")
    post = G.write_model(path, "niw", 8, 6, rng)
    bf = torch.from_numpy(niw_data(post, n, rng).T.copy()).to(DEV).to(torch.bfloat16)      # contiguous (n, D); .T is the (D, n) view
    xh = np.ascontiguousarray(bf.float().cpu().numpy().T)                                  # the same values as a host array
    with host.Predictor.load(path, capacity=256) as p:
        a, b = p.overlap(xh), p.overlap(bf.T)
        want = reference(p, xh)
    assert isinstance(b.matrix, np.ndarray) and isinstance(b.count, np.ndarray)            # K * K numbers: numpy either way
    for f in ("matrix", "mass", "count"):
        assert same(getattr(a, f), getattr(b, f)), f
    check(as_dict(a), want, n, "bf16")
    D, K = 60, 5
    mpath = str(tmp_path / "mult.npz")
    G.write_model(mpath, "mult", D, K, rng)
    csc = sp.csc_matrix(rng.poisson(0.3, (D, n)).astype(np.float32))
    tcsc = torch.sparse_csc_tensor(torch.from_numpy(csc.indptr.astype(np.int64)).to(DEV), torch.from_numpy(csc.indices.astype(np.int64)).to(DEV),
                                   torch.from_numpy(csc.data).to(DEV), size=(D, n))
    with host.Predictor.load(mpath, capacity=256) as p:
        a, b = p.overlap(csc), p.overlap(tcsc)
        want = reference(p, csc)
    for f in ("matrix", "mass", "count"):
        assert same(getattr(a, f), getattr(b, f)), f
    check(as_dict(a), want, n, "csc")


# ------------------------------------------------------------------------------------------------ short slab, points that take no part
def test_the_zero_padding_of_a_short_slab_takes_no_part(host, tmp_path):
    D, K, n, cap = 4, 4, 261, 256
    rng = np.random.default_rng(23)
    path = str(tmp_path / "m.npz")
    post = G.write_model(path, "niw", D, K, rng, zero_mean=True)        # the padding sits at the mean of cluster 1
    X = niw_data(post, n, rng, spread=1.0)
    with host.Predictor.load(path, capacity=n) as p:
        whole = p.overlap(X)
        want = reference(p, X)
    with host.Predictor.load(path, capacity=cap) as p:
        got = p.overlap(X)
        padded = run(p._wk)                                              # what the worker holds now, ranked whole: 5 points and 251 rows of zeros
    check(as_dict(whole), want, n, "capacity n")
    check(as_dict(got), want, n, "capacity 256")
    assert overlap_ref.close(got.matrix, whole.matrix, n) and overlap_ref.close(got.mass, whole.mass, n)
    assert np.array_equal(got.count, whole.count) and got.skipped == whole.skipped == 0 and int(got.count.sum()) == n
    assert padded["count"][0] >= cap - 5 and padded["count"].sum() == cap


def test_points_that_take_no_part_add_nothing(host, tmp_path):
    rng = np.random.default_rng(7)
    n = 261
    path = str(tmp_path / "niw.npz")
    post = G.write_model(path, "niw", 4, 5, rng)
    X = niw_data(post, n, rng)
    X[0, 7] = np.nan                       # a NaN feature: the row of the table is NaN
    X[2, 258] = np.nan
    X[1, 100] = np.inf                     # a +Inf feature: no finite entry
    bad = [7, 100, 258]
    keep = np.setdiff1d(np.arange(n), bad)
    with host.Predictor.load(path, capacity=n) as p:
        got = p.overlap(X)
        lab, P = p.predict(X)
        assert np.isnan(P[bad]).all() and not np.isnan(P[keep]).any()
        clean = p.overlap(np.ascontiguousarray(X[:, keep]))            # the same points without the three
    want = overlap_ref.from_probs(P, lab)
    assert got.skipped == 3 and want["skipped"] == 3 and clean.skipped == 0
    check(as_dict(got), want, n, "niw nan / inf")
    assert overlap_ref.close(got.matrix, clean.matrix, n) and overlap_ref.close(got.mass, clean.mass, n) and np.array_equal(got.count, clean.count)
    # Multinomial: inf * log p = -Inf under every cluster
    D, K = 40, 5
    mpath = str(tmp_path / "mult.npz")
    G.write_model(mpath, "mult", D, K, rng)
    # (0.3 is neither a count nor a bf16 value: both uploads below take the worker's Float32 path.  Plain counts would go through the byte
    # kernel and the data with the Inf through another one, whose table entries differ in the last Float32 bits.)
    C = rng.poisson(0.8, (D, n)).astype(np.float32) + np.float32(0.3) * (rng.random((D, n)) < 0.3)
    C[5, 3] = np.inf
    keep = np.setdiff1d(np.arange(n), [3])
    with host.Predictor.load(mpath, capacity=n) as p:
        got = p.overlap(C)
        lab, P = p.predict(C)
        assert np.isnan(P[3]).all()
        clean = p.overlap(np.ascontiguousarray(C[:, keep]))
    assert got.skipped == 1 and clean.skipped == 0
    check(as_dict(got), overlap_ref.from_probs(P, lab), n, "mult -inf")
    assert overlap_ref.close(got.matrix, clean.matrix, n) and np.array_equal(got.count, clean.count)


def test_a_cluster_that_no_point_chooses(host, tmp_path):
    D, K, n = 4, 5, 261
    rng = np.random.default_rng(21)
    path = str(tmp_path / "m.npz")
    post = G.write_model(path, "niw", D, K, rng)
    post["post_m"][2] += 25.0                                   # cluster 3 sits far from every point, with a heavy tail
    post["post_nu"][2] = D + 3
    np.savez(path, kind=np.int64(0), D=np.int64(D), alpha=np.float64(10.0), points_count=np.full(K, 100.0), **post)
    other = np.delete(post["post_m"], 2, axis=0)
    X = (other[rng.integers(0, K - 1, n)] + rng.standard_normal((n, D))).T.astype(np.float32)
    with host.Predictor.load(path, capacity=n) as p:
        got = p.overlap(X)
        want = reference(p, X)
    check(as_dict(got), want, n, "empty cluster")
    assert got.count[2] == 0 and np.all(got.matrix[2] > 0) and np.all(got.matrix[:, 2] > 0) and 0 < got.mass[2] < 1e-2
    tree = host.merge_tree(got)
    assert tree.merges.shape == (K - 1, 2) and tree.cut(groups=1).tolist() == [1] * K
    lab = np.asarray(want["count"]).argmax() + 1
    assert tree.relabel(torch.full((3,), int(lab), device=DEV), groups=2).device.type == "cuda"


# ------------------------------------------------------------------------------------------------ calls
def test_accumulation_over_calls_reading_twice_beginning_again_and_determinism(pkg):
    wk, tab = G.cached(pkg, "niw64")
    n = wk.n
    wk.overlap_begin()
    wk.overlap_accumulate(500)
    wk.overlap_accumulate(n)                                    # the same upload again, whole
    first, second = wk.overlap_read(), wk.overlap_read()
    want = overlap_ref.add([worker_reference(wk, tab, 500), worker_reference(wk, tab)])
    check(first, want, 500 + n, "two accumulates")
    for k in first:
        assert same(first[k], second[k]), k
    wk.overlap_accumulate(0)                                    # nothing
    third = wk.overlap_read()
    for k in first:
        assert same(first[k], third[k]), k
    one = run(wk)                                               # begin clears
    check(one, worker_reference(wk, tab), n, "begin clears")
    again = run(wk)                                             # the same call: the same bits
    for k in one:
        assert same(one[k], again[k]), k
    # a second pass of the same shape allocates nothing (free bytes unchanged), the read included
    houts = {k: np.empty_like(v) for k, v in one.items()}

    def one_pass():
        wk.overlap_begin()
        wk.overlap_accumulate(n)
        wk.overlap_read_raw(**{k: v.ctypes.data for k, v in houts.items()})
        torch.cuda.synchronize()

    one_pass()
    before = torch.cuda.mem_get_info(0)[0]
    one_pass()
    assert torch.cuda.mem_get_info(0)[0] == before
    for k in one:
        assert same(one[k], houts[k]), k


def test_refusals_come_before_any_launch(pkg):
    n = 300
    rng = np.random.default_rng(3)
    wk = pkg.Worker(pkg.PRIOR_NIW, 2, n, device=0, seed=1)
    wk.upload_points(rng.standard_normal((n, 2)).astype(np.float32))

    def refused(code, fn, *a, what=(), **kw):
        with pytest.raises(pkg.DpmmError) as e:
            fn(*a, **kw)
        assert e.value.code == code, str(e.value)
        for w in what:
            assert w in str(e.value), str(e.value)

    refused(-4, wk.overlap_begin)                                       # DPMM_ESTATE: no predictive parameters yet
    refused(-4, wk.overlap_accumulate, n)                               # no dpmm_overlap_begin
    refused(-4, wk.overlap_read_raw)
    with pytest.raises((RuntimeError, pkg.DpmmError)):
        wk.overlap_read()
    par = S.niw_params(rng, 2, 3)
    wk.set_predictive_niw(*par)
    refused(-4, wk.overlap_accumulate, n)                               # a refused begin starts nothing
    wk.overlap_begin()
    refused(-1, wk.overlap_accumulate, n + 1, what=("n_valid",))
    refused(-1, wk.overlap_accumulate, -1, what=("n_valid",))
    assert wk._lib.dpmm_overlap_read(wk._h, None) == -1                 # out == NULL
    wk.overlap_accumulate(n)
    got = wk.overlap_read()
    assert got["count"].sum() == n and got["skipped"][0] == 0
    wk.set_predictive_niw(*S.niw_params(rng, 2, 4))                    # another K than begin saw
    refused(-4, wk.overlap_accumulate, n, what=("changed",))
    wk.overlap_begin()
    wk.set_predictive_niw(*S.niw_params(rng, 2, 4))                    # the same K, other parameters
    refused(-4, wk.overlap_accumulate, n, what=("changed",))
    assert wk.overlap_read()["count"].sum() == 0                        # nothing was launched: the accumulators are as begin left them
    wk.close()


# ------------------------------------------------------------------------------------------------ missing features, projection
def test_marginalised_points_follow_predict(host, tmp_path):
    D, K, n = 6, 5, 261
    rng = np.random.default_rng(41)
    path = str(tmp_path / "m.npz")
    post = G.write_model(path, "niw", D, K, rng)
    X = niw_data(post, n, rng)
    for i, r in ((3, 1), (64, 2), (200, 3), (260, 1)):                  # points with 1 - 3 NaN features
        X[rng.choice(D, r, replace=False), i] = np.nan
    with host.Predictor.load(path, capacity=256, missing="marginalize") as p:
        got = p.overlap(X)
        assert p.missing_counts == (4, 0)
        want = reference(p, X)
    assert got.skipped == 0 and want["skipped"] == 0
    check(as_dict(got), want, n, "marginalize")
    with host.Predictor.load(path, capacity=256) as p:                  # propagate: the four are skipped
        assert p.overlap(X).skipped == 4


def test_a_projected_model_takes_source_rows(host, tmp_path):
    D_in, d, K, n = 40, 8, 6, 261
    rng = np.random.default_rng(51)
    path = str(tmp_path / "m.npz")
    post = G.write_model(path, "niw", d, K, rng)
    proj = host.random_projection(D_in, d, seed=3)
    np.savez(path, kind=np.int64(0), D=np.int64(d), alpha=np.float64(10.0), points_count=np.full(K, 100.0), **post, **proj.arrays("proj_"))
    Z = niw_data(post, n, rng)                                          # (d, n) in the projected space
    X = (proj.basis @ Z).astype(np.float32)                             # (D_in, n) source rows
    with host.Predictor.load(path, capacity=256) as p:
        assert p.projection is not None
        got = p.overlap(X)
        want = reference(p, X)
    check(as_dict(got), want, n, "projected")
    assert (got.count > 0).sum() >= 2


# ------------------------------------------------------------------------------------------------ poisoned state
def test_overlap_ignores_lds_and_register_contents(pkg, binding):
    """Prep, contraction and reduce kernels under tests/tools/poison.py (their launches go through the library's pre-launch hook): same bits."""
    from tools import poison
    poison.build()
    wk, tab = G.cached(pkg, "niw2", n=261, K=70)
    clean = run(wk)
    with poison.poisoned_kernel_launches(binding, 0xffffffff) as launches:
        dirty = run(wk)
    assert launches[0] >= 4                                            # the sweep, the prep, the contraction, the reduce
    for k in clean:
        assert same(clean[k], dirty[k]), k
    check(dirty, worker_reference(wk, tab), 261, "poisoned")
