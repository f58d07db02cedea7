"""GPU tests of include/dpmm_hip_countholdout.h (csrc/holdout.hip, csrc/countstats_device.h) and of host/score.py's
Predictor.held_out_counts / grow_counts and the floor per count of count_statistics.

The reference is the library's own `score_samples` on the same data and Predictor with the class rule in numpy Float64
(tests/tools/countholdout_ref.py).  Every case first asserts, on the reference values, that no log-density lies within relative 1e-3 of the
raw floor and no log-density per count within relative 1e-3 of the floor per count, that the planted points are all held out and that both
floors hold out points of their own.  Models are written by hand with dyadic alpha: cluster k prefers feature k % (D - 3) and every cluster
gives the last three features the least mass there is, 0.25.  Data: documents of 12 counts drawn from the clusters, every 97th one of 120
counts -- an ordinary long document, which only the raw floor holds out -- and "novel" documents of 12 counts on the last three features,
which only the floor per count holds out, planted on both sides of a wave, a workgroup, a range and a slab boundary.  The floors follow
from the model: log theta of a novel feature is at most max_k log(0.25 / sum alpha_k) =: L, and log w_k <= 0, so a novel document has
logdens / t <= L; fpc = L + 0.5 holds it out, and f = 16 fpc is the same level at a length of 16 counts: above a novel document of 12 counts, below an
ordinary one of 120."""
import ctypes
import functools
import importlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tools import countholdout_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, CAP = 3000, 1024
PLANTED = [0, 255, 256, 1023, 1024, N - 1]
RUN = list(range(1400, 1700))                      # crosses the workgroup boundary at 1536
NAN_AT, INF_AT = 7, 700


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


def as_np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def posterior(D, K, seed=3):
    rng = np.random.default_rng(seed)
    alpha = 0.25 + rng.integers(0, 8, (K, D)) / 4.0                                      # dyadic: exact in Float32
    alpha[:, D - 3:] = 0.25
    for k in range(K):
        alpha[k, k % (D - 3)] += 16.0
    return dict(alpha=alpha.astype(np.float32))


def floors(post):
    a = post["alpha"].astype(np.float64)
    fpc = float(np.log(0.25 / a.sum(1)).max() + 0.5)
    return 16.0 * fpc, fpc


def open_predictor(host, post, cap=CAP, no_u8=False, binding=None, factory=None, prior_alpha=None):
    K, D = post["alpha"].shape
    p = host.Predictor.__new__(host.Predictor)
    p._setup(1, D, 10.0, np.full(K, 100.0), post, cap, 0, factory, prior_alpha=prior_alpha)
    if no_u8:
        p._wk.set_option(binding.OPT_MULT_NO_U8, 1)                                      # before any points: the Float32 store for integer counts
    return p


@functools.lru_cache(maxsize=None)
def dense_data(D, K, n=N, seed=11, gaps=False):
    """(D, n) float32 counts; gaps: one point with a NaN value and one with +Inf (the Float32 and sparse stores)."""
    rng = np.random.default_rng(seed)
    a = posterior(D, K)["alpha"].astype(np.float64)
    z = rng.integers(0, K, n)
    pr = a[z] / a[z].sum(1, keepdims=True)
    X = np.stack([rng.multinomial(120 if i % 97 == 50 else 12, q) for i, q in enumerate(pr)]).astype(np.float32)
    for i in [q for q in PLANTED + RUN if q < n]:
        X[i] = 0
        X[i, D - 3:] = 4
    if gaps:
        X[NAN_AT, 0] = np.nan
        X[INF_AT, 1] = np.inf
    X.setflags(write=False)
    return X.T


def signature(h):
    """The bytes of a HeldOutCounts, whatever its container."""
    pts = h.points
    if isinstance(pts, torch.Tensor) and pts.layout == torch.sparse_csc:
        body = [as_np(pts.ccol_indices()), as_np(pts.row_indices()), as_np(pts.values())]
    elif sp.issparse(pts):
        body = [pts.indptr, pts.indices, pts.data]
    else:
        body = [np.ascontiguousarray(as_np(pts))]
    return tuple(np.ascontiguousarray(b).astype(np.int64 if b.dtype.kind == "i" else b.dtype).tobytes() for b in body) + (as_np(h.index).tobytes(), tuple(h[2:]))


def check(p, data, Xref, f, fpc, what, planted=True, **caps):
    """One held_out_counts call against the reference on score_samples; Xref: numpy (D, n) or scipy CSC, the same points."""
    ld = as_np(p.score_samples(data))
    c = R.classes(ld, Xref, f, fpc)
    fin = np.isfinite(ld)
    assert (np.abs(ld[fin] - np.float32(f)) > 1e-3 * abs(f)).all(), what
    pc = c["complete"] & (c["t"] > 0) & fin
    assert (np.abs(ld[pc].astype(np.float64) / c["t"][pc] - fpc) > 1e-3 * abs(fpc)).all(), what
    raw, per = R.classes(ld, Xref, f, None)["held"], R.classes(ld, Xref, None, fpc)["held"]
    n = len(ld)
    if planted:
        assert c["held"][[q for q in PLANTED + RUN if q < n]].all(), what
        assert (raw & ~per).any() and (per & ~raw).any(), what                          # both floors hold out points of their own
    want = np.flatnonzero(c["held"])
    h = p.held_out_counts(data, min_logdens=f, min_logdens_per_count=fpc, **caps)
    sparse = sp.issparse(Xref)
    lens = np.diff(Xref.indptr)[want] if sparse else np.full(len(want), Xref.shape[0])
    if sparse:
        nnz = int(Xref.indptr[-1])
        stored, stored_entries = R.stored_prefix(lens, min(caps.get("max_points", 1 << 20), n), min(caps.get("max_entries", 1 << 24), nnz))
    else:
        stored = min(caps.get("max_points", 1 << 20), n, caps.get("max_entries", 1 << 24) // Xref.shape[0], len(want))
    idx = as_np(h.index)
    assert idx.dtype == np.int64 and np.array_equal(idx, want[:stored]), what
    assert h.total == len(want) and h.total_entries == int(lens.sum()), what
    if sparse:
        ref = Xref[:, want[:stored]].tocsc()
        if isinstance(h.points, torch.Tensor):
            assert h.points.layout == torch.sparse_csc and h.points.ccol_indices().dtype == h.points.row_indices().dtype == torch.int32, what
            got = [as_np(h.points.ccol_indices()), as_np(h.points.row_indices()), as_np(h.points.values())]
        else:
            assert sp.issparse(h.points) and h.points.format == "csc", what
            got = [h.points.indptr, h.points.indices, h.points.data]
        assert tuple(h.points.shape) == (Xref.shape[0], stored), what
        assert np.array_equal(got[0], ref.indptr) and np.array_equal(got[1], ref.indices), what
        assert got[2].dtype == np.float32 and got[2].tobytes() == ref.data.astype(np.float32).tobytes(), what
        assert int(got[0][-1]) == stored_entries, what
    else:
        got = as_np(h.points)
        assert got.dtype == np.float32 and got.shape == (Xref.shape[0], stored), what
        assert np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(np.asarray(Xref, np.float32)[:, want[:stored]]).tobytes(), what
    cs = p.count_statistics(data, min_logdens=f, min_logdens_per_count=fpc)
    assert (h.total, h.skipped, h.incomplete) == (cs.held_out, cs.skipped, cs.incomplete), what
    assert (cs.held_out, cs.skipped, cs.incomplete) == (int(c["held"].sum()), int(c["skipped"].sum()), int(c["incomplete"].sum())), what
    assert p.count_statistics(data, min_logdens_per_count=fpc).held_out == int(per.sum()), what
    assert int(cs.count.sum()) == int(c["part"].sum()), what
    return h


def torch_csc(X, dev=DEV):
    return torch.sparse_csc_tensor(torch.from_numpy(X.indptr.astype(np.int64)), torch.from_numpy(X.indices.astype(np.int64)), torch.from_numpy(X.data),
                                   size=X.shape).to(dev)


def strided(X, dtype):
    """(D, n) device tensor of `dtype` whose points are 2 D elements apart and whose features 2."""
    D, n = X.shape
    buf = torch.zeros((n, 2 * D), dtype=dtype, device=DEV)
    buf[:, ::2] = torch.tensor(np.ascontiguousarray(X.T)).to(DEV).to(dtype)
    return buf[:, ::2].T


# ------------------------------------------------------------------------------------------------ the stores
STORES = ("byte", "float32", "bfloat16", "int32", "scipy", "tuple", "torch_csc_host", "torch_csc_device")


@pytest.mark.parametrize("store", STORES)
def test_every_store_gives_the_reference_set(host, binding, store):
    D, K = 8, 5
    post = posterior(D, K)
    f, fpc = floors(post)
    gaps = store in ("float32", "scipy", "tuple", "torch_csc_host", "torch_csc_device")
    X = dense_data(D, K, gaps=gaps)
    Xs = sp.csc_matrix(X) if store in STORES[4:] else None
    data = {"byte": lambda: X, "float32": lambda: X, "bfloat16": lambda: strided(X, torch.bfloat16), "int32": lambda: strided(X, torch.int32),
            "scipy": lambda: Xs, "tuple": lambda: (Xs.indptr.astype(np.int64), Xs.indices.astype(np.int64), Xs.data, Xs.shape),
            "torch_csc_host": lambda: torch_csc(Xs, "cpu"), "torch_csc_device": lambda: torch_csc(Xs)}[store]()
    with open_predictor(host, post, no_u8=store == "float32", binding=binding) as p:
        h = check(p, data, Xs if Xs is not None else X, f, fpc, store)
        if store in ("bfloat16", "int32", "torch_csc_device"):
            assert h.points.device == torch.device(DEV) and h.index.device == torch.device(DEV)
        elif store == "torch_csc_host":
            assert h.points.device.type == "cpu"
        elif store in ("scipy", "tuple"):
            assert sp.issparse(h.points) and isinstance(h.index, np.ndarray)
        else:
            assert isinstance(h.points, np.ndarray) and isinstance(h.index, np.ndarray)
        if gaps:                                   # the NaN and the +Inf point are never held out by the floor per count
            held = set(as_np(h.index).tolist())
            assert NAN_AT not in held and INF_AT not in held


# ------------------------------------------------------------------------------------------------ D and K
@pytest.mark.parametrize("D,K", [(300, 5), (8, 1), (8, 70)])
def test_dense_D_and_K(host, binding, D, K):
    post = posterior(D, K)
    f, fpc = floors(post)
    X = dense_data(D, K)
    with open_predictor(host, post) as p:
        check(p, X, X, f, fpc, f"D {D} K {K}")
        check(p, torch.tensor(np.ascontiguousarray(X.T)).to(DEV).T, X, f, fpc, f"D {D} K {K} device")


@functools.lru_cache(maxsize=None)
def wide_sparse(D=65536, K=5, n=N, seed=5):
    """scipy CSC (D, n): ordinary documents of 12 counts, 8 on their cluster's feature and 4 on random rows; long ones of 120; novel ones on the
    last three rows; empty points between held ones; one held column of 700 entries next to columns of 1 or 2; a held point on rows 0, D - 1."""
    rng = np.random.default_rng(seed)
    rows, vals = [], []
    novel = set(q for q in PLANTED + RUN if q < n)
    for i in range(n):
        if i in novel:
            r, v = np.arange(D - 3, D), np.full(3, 4.0)
        else:
            k, scale = int(rng.integers(0, K)), 10 if i % 97 == 50 else 1
            r = np.unique(np.concatenate([[k % (D - 3)], rng.integers(K, D - 3, 4)]))
            v = np.where(r == k % (D - 3), 8.0 * scale, 1.0 * scale)
        rows.append(r)
        vals.append(v)
    for i in (1401, 1403, 1535, 1537, 257):          # empty points between held ones
        rows[i], vals[i] = np.zeros(0, np.int64), np.zeros(0)
    rows[1500], vals[1500] = np.arange(D - 700, D), np.ones(700)          # one held column longer than a workgroup, between short ones
    rows[1499], vals[1499] = np.array([D - 1]), np.array([12.0])
    rows[1501], vals[1501] = np.array([D - 2, D - 1]), np.array([6.0, 6.0])
    rows[2000], vals[2000] = np.array([0, D - 1]), np.array([1.0, 11.0])  # the first and the last row
    cp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return sp.csc_matrix((np.concatenate(vals).astype(np.float32), np.concatenate(rows).astype(np.int64), cp), shape=(D, n))


def test_sparse_D_65536_long_and_empty_columns(host):
    D, K = 65536, 5
    post = posterior(D, K)
    f, fpc = floors(post)
    Xs = wide_sparse()
    with open_predictor(host, post) as p:
        ld = as_np(p.score_samples(Xs))
        c = R.classes(ld, Xs, f, fpc)
        assert c["held"][[1499, 1500, 1501, 2000]].all() and not c["held"][[1401, 1403, 1535, 1537, 257]].any()      # an empty point is never held per count
        check(p, Xs, Xs, f, fpc, "wide scipy", planted=False)
        h = check(p, torch_csc(Xs), Xs, f, fpc, "wide device", planted=False)
        rows = as_np(h.points.row_indices())
        assert rows.min() == 0 and rows.max() == D - 1


# ------------------------------------------------------------------------------------------------ capacity, budget, caps
def test_the_bits_do_not_depend_on_capacity_or_budget(host, binding):
    D, K = 8, 5
    post = posterior(D, K)
    f, fpc = floors(post)
    X = dense_data(D, K, gaps=True)
    Xs = sp.csc_matrix(X)
    for data, ref, no_u8 in ((X, X, True), (dense_data(D, K), dense_data(D, K), False), (torch_csc(Xs), Xs, False)):
        sigs = []
        for cap, mb in ((64, None), (CAP, None), (4096, None), (CAP, 0.01)):          # 0.01 MB: a slab of 1024 points is cut into several ranges
            with open_predictor(host, post, cap=cap, no_u8=no_u8, binding=binding) as p:
                if mb is not None:
                    p._wk.set_option(binding.OPT_SCORE_TABLE_MB, mb)
                sigs.append(signature(p.held_out_counts(data, min_logdens=f, min_logdens_per_count=fpc)))
                if cap == CAP:
                    check(p, data, ref, f, fpc, f"cap {cap} mb {mb}")
        assert all(s == sigs[0] for s in sigs[1:])


def test_caps_keep_the_longest_prefix_inside_both(host):
    D, K = 8, 5
    post = posterior(D, K)
    f, fpc = floors(post)
    X = dense_data(D, K)
    Xs = sp.csc_matrix(X)
    with open_predictor(host, post) as p:
        full = p.held_out_counts(X, min_logdens=f, min_logdens_per_count=fpc)
        assert full.total > 300
        for caps in (dict(max_points=17), dict(max_points=0), dict(max_entries=8 * 40 + 5), dict(max_points=300, max_entries=8 * 1000)):
            h = check(p, X, X, f, fpc, str(caps), **caps)
            assert h.total == full.total
        dev = torch_csc(Xs)
        sfull = p.held_out_counts(dev, min_logdens=f, min_logdens_per_count=fpc)
        lens = np.diff(Xs.indptr)[as_np(sfull.index)]
        cut = int(lens[:50].sum()) + 1                                  # lands inside the 51st held column (every held point has 2 entries or more)
        assert lens[50] >= 2
        for caps in (dict(max_points=17), dict(max_points=0), dict(max_entries=cut), dict(max_entries=0), dict(max_points=60, max_entries=cut),
                     dict(max_points=40, max_entries=cut)):
            h = check(p, dev, Xs, f, fpc, "sparse " + str(caps), **caps)
            assert h.total == sfull.total and h.total_entries == sfull.total_entries
        h = p.held_out_counts(dev, min_logdens=f, min_logdens_per_count=fpc, max_entries=cut)
        assert len(as_np(h.index)) == 50                                # that point and every point behind it are dropped


def test_count_statistics_without_the_keyword_keeps_its_bits(host, binding):
    D, K = 8, 5
    post = posterior(D, K)
    f, fpc = floors(post)
    X = dense_data(D, K, gaps=True)
    Xs = sp.csc_matrix(X)
    for data, no_u8 in ((X, True), (dense_data(D, K), False), (Xs, False)):
        with open_predictor(host, post, no_u8=no_u8, binding=binding) as p, open_predictor(host, post, no_u8=no_u8, binding=binding) as q:
            for mode in ("hard", "soft"):
                p.count_statistics(data, assign=mode, min_logdens=f, min_logdens_per_count=fpc)          # the floor per count does not linger
                a, b = p.count_statistics(data, assign=mode, min_logdens=f), q.count_statistics(data, assign=mode, min_logdens=f)
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:]
                both = p.count_statistics(data, assign=mode, min_logdens=f, min_logdens_per_count=fpc)
                assert both.held_out > a.held_out and int(both.count.sum()) < int(a.count.sum())


# ------------------------------------------------------------------------------------------------ the C boundary
def test_refusals_come_before_any_launch(pkg, host, binding):
    D, K = 8, 5
    post = posterior(D, K)
    f, fpc = floors(post)
    X = dense_data(D, K)
    Xs = sp.csc_matrix(X)
    launches = [0]
    hook_t = ctypes.CFUNCTYPE(None, ctypes.c_void_p)
    cb = hook_t(lambda _arg: launches.__setitem__(0, launches[0] + 1))
    lib = binding.load_library()

    def refused(code, fn, *a, what=()):
        before = launches[0]
        with pytest.raises(pkg.DpmmError) as e:
            fn(*a)
        assert e.value.code == code, str(e.value)
        for w in what:
            assert w in str(e.value), str(e.value)
        assert launches[0] == before, "a kernel was launched before the refusal"

    with open_predictor(host, post, cap=4096) as p:
        wk = p._wk
        p._open(X)[3](0, N)
        dense = dict(points=torch.zeros((16, D), dtype=torch.float32, device=DEV), index=torch.zeros((16,), dtype=torch.int64, device=DEV), cap=16)
        sparse = dict(colptr=torch.ones((17,), dtype=torch.int64, device=DEV), rowval=torch.zeros((64,), dtype=torch.int32, device=DEV),
                      val=torch.zeros((64,), dtype=torch.float32, device=DEV), index=torch.zeros((16,), dtype=torch.int64, device=DEV), cap=16, entry_cap=64)
        lib.dpmm_debug_set_prelaunch_hook(ctypes.cast(cb, ctypes.c_void_p), None)
        try:
            refused(-4, wk.countholdout_accumulate, 0, N, what=("dpmm_countholdout_begin",))      # DPMM_ESTATE: no begin
            refused(-4, wk.countholdout_read)
            refused(-1, wk.countholdout_begin, dense, what=("floor",))                            # DPMM_EINVAL: no floor
            refused(-4, wk.countholdout_accumulate, 0, N)                                         # a refused begin starts nothing
            refused(-1, wk.countholdout_begin, dense, None, float("nan"), what=("NaN",))
            refused(-1, wk.countholdout_begin, dict(dense, cap=-1), f, what=("cap",))
            refused(-1, wk.countholdout_begin, dict(dense, colptr=sparse["colptr"]), f, what=("not both",))
            refused(-1, wk.countholdout_begin, dict(index=dense["index"], cap=16), f, what=("destination",))
            refused(-1, wk.countholdout_begin, dict(dense, points=np.zeros((16, D), np.float32).ctypes.data), f, what=("dst_points",))
            wk.countholdout_begin(sparse, f, fpc)                                                  # a sparse destination, a dense store live
            assert int(sparse["colptr"][0]) == 0                                                   # slot 0 is written by begin
            refused(-4, wk.countholdout_accumulate, 0, N, what=("dense store is live",))
            wk.countholdout_begin(dense, f, fpc)
            refused(-1, wk.countholdout_accumulate, 0, 4097, what=("n_valid",))
            refused(-1, wk.countholdout_accumulate, -1, N, what=("indices",))
            assert lib.dpmm_countholdout_read(wk._h, None) == -1                                   # out == NULL
            p._open(Xs)[3](0, N)                                                                   # now the sparse store is live
            refused(-4, wk.countholdout_accumulate, 0, N, what=("sparse store is live",))
            p._open(X)[3](0, N)
            before = launches[0]
            wk.countholdout_accumulate(0, N)                                                       # the ctx is usable afterwards
            assert launches[0] > before
            seen = wk.countholdout_read()
            assert seen["stored"] == 16 and seen["total"] >= len(PLANTED) + len(RUN) and seen["stored_entries"] == 16 * D
            assert seen["total"] + seen["skipped"] + seen["incomplete"] + seen["scored"] == N
            # the floor per count of the statistics: between begin and the first accumulate
            refused(-4, wk.countstats_set_per_count, fpc, what=("dpmm_countstats_begin",))
            wk.countstats_begin(binding.BATCHSTATS_HARD, f)
            refused(-1, wk.countstats_set_per_count, float("nan"), what=("NaN",))
            wk.countstats_set_per_count(fpc)
            wk.countstats_accumulate(N)
            refused(-4, wk.countstats_set_per_count, fpc, what=("between",))
            r = wk.countstats_read()
            assert (int(r["held_out"][0]), int(r["skipped"][0]), int(r["incomplete"][0])) == (seen["total"], seen["skipped"], seen["incomplete"])
            which, args = p._predictive_args()
            wk.set_predictive_mult(*args)                                                          # the parameters loaded again
            refused(-4, wk.countholdout_accumulate, 0, N, what=("changed",))
        finally:
            lib.dpmm_debug_set_prelaunch_hook(None, None)
    niw = pkg.Worker(pkg.PRIOR_NIW, 8, 100, device=0, seed=1)
    refused(-1, niw.countholdout_begin, None, f, what=("Multinomial",))                            # DPMM_EINVAL, whatever its state
    niw.close()
    mult = pkg.Worker(pkg.PRIOR_MULT, 8, 100, device=0, seed=1)
    refused(-4, mult.countholdout_begin, None, f, what=("dpmm_set_predictive_mult",))              # DPMM_ESTATE: no predictive parameters yet
    mult.close()


# ------------------------------------------------------------------------------------------------ grow_counts
GD, GK, GOLD, GNEW, TRIALS = 24, 3, 2000, 300, 40
GFPC = -3.5


def grow_post():
    alpha = np.full((GK, GD), 0.25)
    for k in range(GK):
        alpha[k, 4 * k:4 * k + 4] = 8.0
    return dict(alpha=alpha.astype(np.float32))


def grow_data(p):
    """(D, n) device tensor: 2000 draws of the model, then 300 documents of each of two novel topics on features 12..17 and 18..23."""
    old, _ = p.sample(GOLD, seed=4, trials=TRIALS)
    rng = np.random.default_rng(21)
    new = np.zeros((2 * GNEW, GD), np.float32)
    new[:GNEW, 12:18] = rng.multinomial(TRIALS, np.full(6, 1 / 6), GNEW)
    new[GNEW:, 18:24] = rng.multinomial(TRIALS, np.full(6, 1 / 6), GNEW)
    return torch.cat([old.T.contiguous(), torch.from_numpy(new).to(DEV)]).T


def post_bytes(p):
    return {k: v.tobytes() for k, v in p.post.items()}, p.points_count.tobytes(), p.weights.tobytes(), p.K


@pytest.mark.parametrize("layout", ["dense", "sparse_csc"])
def test_grow_counts_appends_the_two_novel_topics(host, layout, tmp_path):
    with open_predictor(host, grow_post(), cap=1024, prior_alpha=np.ones(GD)) as p:
        X = grow_data(p)
        data = X if layout == "dense" else X.T.contiguous().T.to_sparse_csc()
        n = GOLD + 2 * GNEW
        per = as_np(p.score_samples(data)).astype(np.float64) / TRIALS
        assert per[:GOLD].min() > GFPC + 0.1 and per[GOLD:].max() < GFPC - 0.1          # the gap the floor sits in
        before = post_bytes(p)
        g = p.grow_counts(data, min_logdens_per_count=GFPC, seed=0)
        assert isinstance(g, host.Growth) and g.added >= 2 and g.total == 2 * GNEW and p.K == GK + g.added
        assert np.array_equal(np.sort(g.index), g.index) and g.index.min() >= GOLD
        for j in range(g.added):                                                         # every new cluster: documents of one novel topic only
            members = g.index[g.labels == GK + 1 + j]
            assert len(members) == g.sizes[j] >= 10
            assert (members < GOLD + GNEW).all() or (members >= GOLD + GNEW).all()
        assert p.post["alpha"].dtype == np.float64 and p.post["alpha"].shape == (GK + g.added, GD)
        assert p.post["alpha"][:GK].astype(np.float32).tobytes() == before[0]["alpha"]   # the old rows and numbers
        assert p.points_count[:GK].tobytes() == before[1] and np.array_equal(p.points_count[GK:], g.sizes.astype(np.float64))
        lab = as_np(p.predict_labels(data))
        assert (lab[:GOLD] <= GK).all() and (lab[GOLD:] > GK).all()
        topic = [set(lab[GOLD:GOLD + GNEW].tolist()), set(lab[GOLD + GNEW:].tolist())]
        assert not topic[0] & topic[1]
        drawn, dl = p.sample(500, seed=9, trials=TRIALS)                                 # sample works with the new K
        assert tuple(drawn.shape) == (GD, 500) and int(dl.max()) <= p.K and int(dl.max()) > GK
        path = str(tmp_path / "grown.npz")
        p.save(path)
        want = as_np(p.score_samples(data))
        with host.Predictor.load(path, device=0, capacity=1024) as q:
            assert q.K == p.K and np.array_equal(q.prior_alpha, np.ones(GD))
            assert as_np(q.score_samples(data)).tobytes() == want.tobytes()
        assert n == len(want)
        again = p.count_statistics(data, min_logdens_per_count=GFPC)                     # the grown model explains the batch
        assert again.held_out == 0


def test_a_failing_reload_leaves_the_predictor_as_it_was(host, binding):
    class Failing(binding.Worker):
        loads = 0

        def set_predictive_mult(self, *a, **kw):
            Failing.loads += 1
            if Failing.loads > 1:
                raise RuntimeError("injected: the reload failed")
            return super().set_predictive_mult(*a, **kw)
    with open_predictor(host, grow_post(), cap=1024, factory=Failing, prior_alpha=np.ones(GD)) as p:
        X = grow_data(p)
        before = post_bytes(p)
        with pytest.raises(RuntimeError, match="injected"):
            p.grow_counts(X, min_logdens_per_count=GFPC, seed=0)
        assert post_bytes(p) == before and Failing.loads == 2
        assert p.count_statistics(X, min_logdens_per_count=GFPC).held_out == 2 * GNEW     # the worker still serves the old model


# ------------------------------------------------------------------------------------------------ a range of more than 256 workgroups
def test_a_range_of_more_than_256_workgroups(host, binding):
    """One range of n = 256 * 256 + 257 points of the Float32 store: 258 workgroups, so a thread of the one scan workgroup owns two of them.
    Novel documents lie on both sides of the piece boundaries 65535 | 65536 and 65791 | 65792, at both ends and at every 997th point; one
    floor, the floor per count.  The expected set is the class rule on `score_samples` of the same Predictor, under the precondition of `check`."""
    D, K, n = 5, 1, 256 * 256 + 257
    planted = sorted({0, 65535, 65536, 65791, 65792, n - 1} | set(range(500, n, 997)))      # ... and one in most threads' pieces
    nan_at = 40000
    post = posterior(D, K)
    _, fpc = floors(post)
    a = post["alpha"][0].astype(np.float64)
    X = np.random.default_rng(13).multinomial(12, a / a.sum(), size=n).astype(np.float32)
    X[planted] = 0
    X[planted, D - 3:] = 4
    X[nan_at, 0] = np.nan
    X = np.ascontiguousarray(X.T)                                                  # (D, n)
    with open_predictor(host, post, cap=1 << 17, no_u8=True, binding=binding) as p:      # one short slab, one range
        ld = as_np(p.score_samples(X))
        h = p.held_out_counts(X, min_logdens_per_count=fpc, max_points=n)
    c = R.classes(ld, X, None, fpc)
    pc = c["complete"] & (c["t"] > 0) & np.isfinite(ld)
    assert (np.abs(ld[pc].astype(np.float64) / c["t"][pc] - fpc) > 1e-3 * abs(fpc)).all()
    want = np.flatnonzero(c["held"]).astype(np.int64)
    assert c["held"][planted].all() and not c["held"][nan_at]
    print(f"n = {n}: held out {h.total} (reference {len(want)}), skipped {h.skipped}, incomplete {h.incomplete}")
    assert as_np(h.index).dtype == np.int64 and np.array_equal(as_np(h.index), want)
    got = as_np(h.points)
    assert got.dtype == np.float32 and np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(X[:, want]).tobytes()
    assert (h.total, h.total_entries) == (len(want), D * len(want))
    assert (h.skipped, h.incomplete) == (int(c["skipped"].sum()), int(c["incomplete"].sum())) and h.skipped == 1
    with open_predictor(host, post, cap=1024, no_u8=True, binding=binding) as p:         # 65 slabs: the same bytes
        assert signature(p.held_out_counts(X, min_logdens_per_count=fpc, max_points=n)) == signature(h)
