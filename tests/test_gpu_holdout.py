"""GPU tests of include/dpmm_hip_holdout.h (csrc/holdout.hip) and of host/score.py's Predictor.held_out / grow.

The models are written by hand and served through `Predictor.load`: K clusters of unit scale 30 apart.  The data: n = 3000 draws around
them (three slabs of capacity 1024, the last one short) with far points planted at 0, 255, 256, 1023, 1024 and n - 1 -- a held-out point
on both sides of a wave, a workgroup, a range and a slab boundary -- a run of 300 consecutive far points, one NaN row and one +Inf feature.

The reference is what the library had before this header: a point is held out when `typicality(data).tail < t` (complete points; the tail
of any other is NaN and compares false) or `score_samples(data) < f` (a log-density that is not finite belongs to a skipped point, which
the rule of `statistics` classes first); the counters are those of `statistics(data, min_tail=t, min_logdens=f)`.  Each case asserts, on
the reference values, that no tail lies within relative 1e-3 of t and no log-density within 1e-3 of f: t = 1e-4 is fixed, f is the middle
of the widest gap between neighbouring log-densities around the 40th lowest of the points the tail keeps, so that the floor holds out
points of its own."""
import ctypes
import functools
import importlib
import os
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 3000
CAP = 1024
TILE = 256                            # points per tile of the score table for D <= 64: the smallest range
T = 1e-4
PLANTED = [0, 255, 256, 1023, 1024, N - 1]
RUN = list(range(1400, 1700))         # crosses the workgroup boundary at 1536
NAN_ROW, INF_ROW = 700, 701
CASES = [(D, K) for D in (5, 36, 64) for K in (1, 3)]


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


def means(D, K):
    m = np.zeros((K, D))
    for k in range(1, K):
        m[k, (k - 1) % D] = 30.0
    return m


def model_file(D, K, prior=True):
    """A served model written by hand: K clusters of unit scale at `means`, 200 points each; psi = I, so U = sqrt(nu) I and logdet_psi = 0."""
    nu = np.full(K, 200.0 + D)
    arrays = dict(kind=np.int64(0), D=np.int64(D), alpha=np.float64(10.0), points_count=np.full(K, 200.0), post_kappa=np.full(K, 200.0), post_nu=nu,
                  post_m=means(D, K), post_U=np.sqrt(nu)[:, None, None] * np.eye(D)[None], post_logdet_psi=np.zeros(K))
    if prior:
        arrays.update(prior_kappa=np.float64(1.0), prior_m=np.zeros(D), prior_nu=np.float64(D + 3.0), prior_psi=np.eye(D))
    path = os.path.join(tempfile.mkdtemp(prefix="holdout_"), f"model_{D}_{K}.npz")
    np.savez(path, **arrays)
    return path


def as_np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def bits(h):
    """What a HeldOut must reproduce to the bit."""
    return (np.ascontiguousarray(as_np(h.points)).tobytes(), tuple(h.points.shape), as_np(h.index).tobytes(), h.total, h.skipped, h.incomplete)


def budget_one_tile(K):
    """MB of one tile of an NIW table: the smallest budget, it cuts a slab of 1024 points into four ranges."""
    return K * TILE * 4 / 2.0 ** 20


@functools.lru_cache(maxsize=None)
def case(D, K, dtype):
    """The data (a device tensor of `dtype`), the model file and the reference of one shape: computed once, shared, left unchanged."""
    from __graft_entry__ import load_package
    host = importlib.import_module(load_package().__name__ + ".host")
    rng = np.random.default_rng(100 * D + K)
    m = means(D, K)
    X = (m[rng.integers(0, K, N)] + rng.standard_normal((N, D))).astype(np.float32)
    far = PLANTED + RUN
    X[far] = (100.0 + 5.0 * rng.standard_normal((len(far), D))).astype(np.float32)
    X[NAN_ROW] = np.nan
    X[INF_ROW, 0] = np.inf
    data = torch.from_numpy(X).to(DEV).to(getattr(torch, dtype)).T             # (D, N), point-major memory
    path = model_file(D, K)
    with host.Predictor.load(path, device=0, capacity=CAP) as p:
        tail = as_np(p.typicality(data).tail)
        ld = as_np(p.score_samples(data))
        with np.errstate(invalid="ignore"):
            by_tail = tail < np.float32(T)
        rest = np.sort(ld[np.isfinite(ld) & ~by_tail])
        j = 20 + int(np.argmax(np.diff(rest[20:61])))
        f = float(np.float32(0.5 * (float(rest[j]) + float(rest[j + 1]))))
        with np.errstate(invalid="ignore"):
            held = by_tail | (np.isfinite(ld) & (ld < np.float32(f)))
        stats = p.statistics(data, min_tail=T, min_logdens=f)
    # the precondition: no complete point's tail within relative 1e-3 of t, no log-density within 1e-3 of f
    ok = np.isfinite(tail)
    assert np.all(np.abs(tail[ok] - T) > 1e-3 * T), "a tail too close to the floor: another seed"
    assert np.all(np.abs(ld[np.isfinite(ld)] - f) > 1e-3), "a log-density too close to the floor: another seed"
    assert held[far].all() and 20 <= int(held.sum()) - len(far) <= 65 and not held[[NAN_ROW, INF_ROW]].any()
    return dict(data=data, path=path, f=f, index=np.flatnonzero(held).astype(np.int64), stats=stats)


# ------------------------------------------------------------------------------------------------ the held-out set
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("D,K", CASES)
def test_held_out_equals_the_reference_set_and_the_counters_of_statistics(host, D, K, dtype):
    c = case(D, K, dtype)
    with host.Predictor.load(c["path"], device=0, capacity=CAP) as p:
        h = p.held_out(c["data"], min_tail=T, min_logdens=c["f"])
    assert isinstance(h, host.HeldOut) and h.points.device == c["data"].device and h.index.device == c["data"].device
    assert h.points.dtype == torch.float32 and h.index.dtype == torch.int64 and tuple(h.points.shape) == (D, len(c["index"]))
    assert h.points.T.is_contiguous()                                          # a view of the (stored, D) buffer
    assert np.array_equal(as_np(h.index), c["index"])
    want = c["data"].float()[:, torch.from_numpy(c["index"]).to(DEV)]
    assert np.ascontiguousarray(as_np(h.points)).tobytes() == np.ascontiguousarray(as_np(want)).tobytes()
    s = c["stats"]
    print(f"D = {D} K = {K} {dtype}: held out {h.total} (statistics {s.held_out}), skipped {h.skipped} ({s.skipped}), incomplete {h.incomplete} ({s.incomplete})")
    assert (h.total, h.skipped, h.incomplete) == (s.held_out, s.skipped, s.incomplete) and h.skipped == 2
    assert h.total == len(c["index"])


@pytest.mark.parametrize("D,K", CASES)
def test_the_bits_do_not_depend_on_capacity_budget_or_where_the_data_lies(host, binding, D, K):
    c = case(D, K, "float32")
    kw = dict(min_tail=T, min_logdens=c["f"])
    with host.Predictor.load(c["path"], device=0, capacity=CAP) as p:
        base = bits(p.held_out(c["data"], **kw))
        assert bits(p.held_out(c["data"], **kw)) == base                     # a second call on the same Predictor
        on_host = p.held_out(c["data"].cpu().numpy(), **kw)
        assert isinstance(on_host.points, np.ndarray) and isinstance(on_host.index, np.ndarray) and bits(on_host) == base
        p._wk.set_option(binding.OPT_SCORE_TABLE_MB, budget_one_tile(K))      # four ranges per slab
        assert bits(p.held_out(c["data"], **kw)) == base
        assert bits(p.held_out(c["data"].cpu().numpy(), **kw)) == base
    with host.Predictor.load(c["path"], device=0, capacity=4096) as p:        # one short slab of 3000 points
        assert bits(p.held_out(c["data"], **kw)) == base
        p._wk.set_option(binding.OPT_SCORE_TABLE_MB, budget_one_tile(K))
        assert bits(p.held_out(c["data"], **kw)) == base


# ------------------------------------------------------------------------------------------------ edge cases
def test_nobody_everybody_and_a_destination_smaller_than_the_set(host, binding):
    D, K = 5, 3
    c = case(D, K, "float32")
    data = c["data"]
    with host.Predictor.load(c["path"], device=0, capacity=CAP) as p:
        h = p.held_out(data, min_logdens=-1e30)                                # nobody lies below
        assert h.total == 0 and tuple(h.points.shape) == (D, 0) and tuple(h.index.shape) == (0,) and h.skipped == 2
        h = p.held_out(data, min_logdens=1e30)                                 # everybody that is not skipped
        everybody = np.delete(np.arange(N), [NAN_ROW, INF_ROW])
        assert h.total == N - 2 and np.array_equal(as_np(h.index), everybody)
        assert as_np(h.points).tobytes() == np.ascontiguousarray(as_np(data.float()[:, torch.from_numpy(everybody).to(DEV)])).tobytes()
        h = p.held_out(data, min_tail=1.0, max_points=0)                       # counted only
        assert h.total > 7 and tuple(h.points.shape) == (D, 0)
        h = p.held_out(data, min_tail=T, min_logdens=c["f"], max_points=7)
        assert h.total == len(c["index"]) > 7 and np.array_equal(as_np(h.index), c["index"][:7]) and tuple(h.points.shape) == (D, 7)
        assert as_np(h.points).tobytes() == np.ascontiguousarray(as_np(data.float()[:, torch.from_numpy(c["index"][:7]).to(DEV)])).tobytes()
    # at the binding level: nothing is written beyond slot 6 of an oversized buffer
    with host.Predictor.load(c["path"], device=0, capacity=4096) as p:
        wk = p._wk
        p._open(data)[3](0, N)                                                 # the worker's points: the 3000, zero padded
        for budget in (-1, budget_one_tile(K)):
            wk.set_option(binding.OPT_SCORE_TABLE_MB, budget)
            pts = torch.full((64, D), -7.25, dtype=torch.float32, device=DEV)
            idx = torch.full((64,), -99, dtype=torch.int64, device=DEV)
            wk.holdout_begin(pts, idx, 7, c["f"], T)
            wk.holdout_accumulate(0, 1500)                                     # n_valid inside a range, the rest in a second call
            r = wk.holdout_read()
            assert r["stored"] == 7 and r["total"] == int((c["index"] < 1500).sum())
            wk.holdout_accumulate(0, N)
            r = wk.holdout_read()
            assert r["stored"] == 7 and r["total"] == int((c["index"] < 1500).sum()) + len(c["index"])
            assert r["total"] + r["skipped"] + r["incomplete"] + r["scored"] == 1500 + N
            assert np.array_equal(as_np(idx[:7]), c["index"][:7]) and (as_np(idx[7:]) == -99).all() and (as_np(pts[7:]) == -7.25).all()
            assert as_np(pts[:7]).tobytes() == np.ascontiguousarray(as_np(data.float().T[torch.from_numpy(c["index"][:7]).to(DEV)])).tobytes()


def test_uploads_chain_and_global_indices_follow_lo(host, binding):
    """Two uploads of the same points under one begin: the second one's points follow the first one's, with indices lo + i."""
    D, K = 36, 3
    c = case(D, K, "float32")
    n_held = len(c["index"])
    with host.Predictor.load(c["path"], device=0, capacity=4096) as p:
        wk = p._wk
        p._open(c["data"])[3](0, N)
        pts = torch.zeros((2 * n_held, D), dtype=torch.float32, device=DEV)
        idx = torch.zeros((2 * n_held,), dtype=torch.int64, device=DEV)
        wk.holdout_begin(pts, idx, 2 * n_held, c["f"], T)
        wk.holdout_accumulate(0, N)
        wk.holdout_accumulate(5_000_000_000, N)                                # indices beyond 2^32
        r = wk.holdout_read()
        assert r["total"] == r["stored"] == 2 * n_held
        assert np.array_equal(as_np(idx), np.concatenate([c["index"], c["index"] + 5_000_000_000]))
        assert as_np(pts[:n_held]).tobytes() == as_np(pts[n_held:]).tobytes()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_launch(pkg, host, binding):
    D, K = 5, 3
    c = case(D, K, "float32")
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

    with host.Predictor.load(c["path"], device=0, capacity=4096) as p:
        wk = p._wk
        p._open(c["data"])[3](0, N)
        pts = torch.zeros((16, D), dtype=torch.float32, device=DEV)
        idx = torch.zeros((16,), dtype=torch.int64, device=DEV)
        lib.dpmm_debug_set_prelaunch_hook(ctypes.cast(cb, ctypes.c_void_p), None)
        try:
            refused(-4, wk.holdout_accumulate, 0, N, what=("dpmm_holdout_begin",))          # DPMM_ESTATE: no begin
            refused(-4, wk.holdout_read)
            refused(-1, wk.holdout_begin, pts, idx, 16, what=("floor",))                     # DPMM_EINVAL: no floor
            refused(-4, wk.holdout_accumulate, 0, N)                                         # a refused begin starts nothing
            refused(-1, wk.holdout_begin, pts, idx, 16, None, 0.0, what=("min_tail",))
            refused(-1, wk.holdout_begin, pts, idx, 16, None, 1.5, what=("min_tail",))
            refused(-1, wk.holdout_begin, pts, idx, -1, None, T, what=("cap",))
            refused(-1, wk.holdout_begin, pts.cpu().numpy().ctypes.data, idx, 16, None, T, what=("dst_points",))
            wk.holdout_begin(pts, idx, 16, None, T)
            refused(-1, wk.holdout_accumulate, 0, 4097, what=("n_valid",))
            refused(-1, wk.holdout_accumulate, 0, -1, what=("n_valid",))
            refused(-1, wk.holdout_accumulate, -1, N, what=("indices",))
            assert lib.dpmm_holdout_read(wk._h, None) == -1                                  # out == NULL
            before = launches[0]
            wk.holdout_accumulate(0, 0)                                                      # nothing
            assert launches[0] == before
            wk.holdout_accumulate(0, N)
            assert launches[0] > before
            seen = wk.holdout_read()
            assert seen["stored"] == 16 and seen["total"] >= len(PLANTED) + len(RUN)
            which, args = p._predictive_args()
            wk.set_predictive_niw(*args)                                                     # the same K, the parameters loaded again
            refused(-4, wk.holdout_accumulate, 0, N, what=("changed",))
            assert wk.holdout_read() == seen                                                 # nothing was launched: the counters are as they were
        finally:
            lib.dpmm_debug_set_prelaunch_hook(None, None)
    mult = pkg.Worker(pkg.PRIOR_MULT, 8, 100, device=0, seed=1)
    refused(-1, mult.holdout_begin, 0, 0, 0, None, T, what=("Multinomial",))                 # DPMM_EINVAL, whatever its state
    mult.close()


# ------------------------------------------------------------------------------------------------ grow
GD, GBLOB = 8, 300


@functools.lru_cache(maxsize=None)
def grow_data():
    rng = np.random.default_rng(77)
    m = means(GD, 2)
    near = (m[rng.integers(0, 2, 700)] + rng.standard_normal((700, GD))).astype(np.float32)
    blob = rng.standard_normal((GBLOB, GD)).astype(np.float32)
    blob[:, 2] += 60.0                                                         # far from both
    X = np.concatenate([near[:400], blob, near[400:]])
    return torch.from_numpy(X).to(DEV).T, np.arange(400, 400 + GBLOB), np.concatenate([np.arange(400), np.arange(400 + GBLOB, 700 + GBLOB)])


def post_bytes(p):
    return {k: v.tobytes() for k, v in p.post.items()}, p.points_count.tobytes(), p.weights.tobytes(), p.K


def test_grow_appends_the_blob_as_a_third_cluster(host):
    data, blob, near = grow_data()
    path = model_file(GD, 2)
    with host.Predictor.load(path, device=0, capacity=CAP) as p:
        assert p.held_out(data, min_tail=T).total == GBLOB, "a near point below the floor: another seed"
        before = post_bytes(p)
        old_labels, old_probs = (as_np(a) for a in p.predict(data[:, torch.from_numpy(near).to(DEV)]))
        g = p.grow(data[:, torch.from_numpy(near).to(DEV)], min_logdens=-1e30)      # nothing beyond the floor: nothing changes
        assert (g.added, g.total, g.dropped, g.model) == (0, 0, 0, None) and post_bytes(p) == before
        g = p.grow(data, min_tail=T)
        print("grow: added", g.added, "sizes", g.sizes, "dropped", g.dropped, "total", g.total, "sub-fit K", g.model.sampler.K)
        assert isinstance(g, host.Growth) and g.added == 1 and g.total == GBLOB and p.K == 3
        assert int(g.sizes[0]) + g.dropped == GBLOB and len(g.index) == int(g.sizes[0]) and (g.labels == 3).all()
        assert np.isin(g.index, blob).all() and np.all(np.diff(g.index) > 0)
        for k, v in p.post.items():                                            # the old rows keep their bits
            assert v[:2].tobytes() == before[0][k], k
        assert p.points_count[:2].tobytes() == before[1] and p.points_count[-1] == float(g.sizes[0])
        sub = g.model.sampler
        sizes = np.bincount(as_np(g.model.labels).astype(np.int64) - 1, minlength=sub.K)
        kept = np.flatnonzero(sizes >= GD + 1)
        assert len(kept) == 1 and sizes[kept[0]] == g.sizes[0]
        for k in ("kappa", "nu", "m", "U", "logdet_psi"):
            assert p.post[k][2:].tobytes() == np.asarray(sub.post[k], np.float64)[3 * kept].tobytes(), k
        assert p.weights.dtype == np.float32 and len(p.weights) == 3 and abs(float(p.weights.astype(np.float64).sum()) - 1.0) <= 3 * 2.0 ** -24
        assert (as_np(p.predict_labels(data[:, torch.from_numpy(g.index).to(DEV)])) == 3).all()
        new_labels, _ = p.predict(data[:, torch.from_numpy(near).to(DEV)])
        assert np.array_equal(as_np(new_labels), old_labels)
        saved = os.path.join(os.path.dirname(path), "grown.npz")
        p.save(saved)
        lab, probs = (as_np(a) for a in p.predict(data))
        x, z = p.sample(200, seed=3)
        assert tuple(x.shape) == (GD, 200) and int(z.min()) >= 1 and int(z.max()) <= 3 and torch.isfinite(x).all()
        assert p.held_out(data, min_tail=T).total < GBLOB                      # the blob is explained now
    with host.Predictor.load(saved, device=0, capacity=CAP) as q:
        assert q.K == 3 and q.prior_hyper is not None
        lab2, probs2 = (as_np(a) for a in q.predict(data))
        assert lab2.tobytes() == lab.tobytes() and probs2.tobytes() == probs.tobytes()
    with host.Predictor.load(path, device=0, capacity=CAP) as r:               # every sub-cluster is smaller than min_points
        before = post_bytes(r)
        g = r.grow(data, min_tail=T, min_points=GBLOB + 1)
        assert g.added == 0 and g.dropped == GBLOB and g.total == GBLOB and post_bytes(r) == before and r.K == 2
    with host.Predictor.load(model_file(GD, 2, prior=False), device=0, capacity=CAP) as r:      # a file without the prior
        with pytest.raises(ValueError, match="prior="):
            r.grow(data, min_tail=T)
        g = r.grow(data, min_tail=T, prior=host.niw_hyperparams(1.0, np.zeros(GD), GD + 3.0, np.eye(GD)))
        assert g.added == 1 and r.K == 3


# ------------------------------------------------------------------------------------------------ a range of more than 256 workgroups
def test_a_range_of_more_than_256_workgroups(host):
    """One range of n = 256 * 256 + 257 points: 258 workgroups, so a thread of the one scan workgroup owns two of them.  Far points lie on
    both sides of the piece boundaries 65535 | 65536 and 65791 | 65792, at both ends and at every 997th point; one floor, min_tail = 1e-4.  The expected set comes
    from `typicality` and `score_samples` of the same Predictor, under the precondition of `case`: no tail within relative 1e-3 of t."""
    D, K, n = 5, 1, 256 * 256 + 257
    planted = sorted({0, 65535, 65536, 65791, 65792, n - 1} | set(range(500, n, 997)))      # ... and one in most threads' pieces
    nan_row = 40000
    rng = np.random.default_rng(7)
    X = rng.standard_normal((n, D)).astype(np.float32)
    X[planted] = (100.0 + 5.0 * rng.standard_normal((len(planted), D))).astype(np.float32)
    X[nan_row] = np.nan
    data = torch.from_numpy(X).to(DEV).T
    path = model_file(D, K)
    with host.Predictor.load(path, device=0, capacity=1 << 17) as p:            # one short slab, one range
        tail = as_np(p.typicality(data).tail)
        ld = as_np(p.score_samples(data))
        h = p.held_out(data, min_tail=T, max_points=n)
    ok = np.isfinite(tail)
    assert np.all(np.abs(tail[ok] - T) > 1e-3 * T), "a tail too close to the floor: another seed"
    with np.errstate(invalid="ignore"):
        held = tail < np.float32(T)
    want = np.flatnonzero(held).astype(np.int64)
    assert held[planted].all() and not held[nan_row]
    print(f"n = {n}: held out {h.total} (reference {len(want)}), skipped {h.skipped}, incomplete {h.incomplete}")
    assert as_np(h.index).dtype == np.int64 and np.array_equal(as_np(h.index), want)
    assert np.ascontiguousarray(as_np(h.points)).tobytes() == np.ascontiguousarray(X[want].T).tobytes()
    assert (h.total, h.skipped, h.incomplete) == (len(want), int((~np.isfinite(ld)).sum()), 0) and h.skipped == 1
    with host.Predictor.load(path, device=0, capacity=1024) as p:               # 65 slabs: the same bytes
        assert bits(p.held_out(data, min_tail=T, max_points=n)) == bits(h)
