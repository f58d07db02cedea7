"""GPU tests of include/dpmm_hip_trace.h (csrc/trace.hip) and of the posterior summary on top of it (host/summary.py).

Labels are fed with `Worker.set_labels` and recorded with `trace_record`; no points are uploaded, the trace reads none.  Tables are
integers and are compared with `numpy.bincount` for EQUALITY.  The confidence is compared with Float64 numpy under the derived bound
(T + 2) * 2^-24 absolute: T terms in [0, 1] each rounded once to Float32 (2^-25 each, 2^-25 after the mean), T - 1 Float32 additions
of partial sums <= T (T * 2^-24 each at most, (T - 1) * 2^-24 after the mean), one division with a result <= 1 (2^-25)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from tools.summary_ref import binder_numpy, check_summary_recomputes, vi_numpy

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL, ESTATE = -1, -4


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


@pytest.fixture(scope="module")
def summary(pkg):
    return importlib.import_module(pkg.__name__ + ".host.summary")


def worker(binding, n, ids=(), K=(), slots=None):
    """A worker of n points whose trace holds the 0-based labellings `ids` with `K` clusters each."""
    wk = binding.Worker(binding.PRIOR_NIW, 2, n, device=0, seed=1)
    wk.trace_open(len(ids) if slots is None else slots)
    for j, (z, k) in enumerate(zip(ids, K)):
        wk.set_labels(np.asarray(z, np.int64) + 1, np.ones(n, np.int64))
        wk.trace_record(j, k)
    return wk


def want(za, zb, Ka, Kb):
    za, zb = np.asarray(za, np.int64), np.asarray(zb, np.int64)
    ok = (za < Ka) & (zb < Kb)
    return np.bincount(za[ok] * Kb + zb[ok], minlength=Ka * Kb).reshape(Ka, Kb)


def check_tables(got, pairs, ids, K):
    assert len(got) == len(pairs)
    for t, (a, b) in zip(got, pairs):
        assert t.dtype == np.int64 and t.shape == (K[a], K[b]) and np.array_equal(t, want(ids[a], ids[b], K[a], K[b])), (a, b)


def test_tables_of_every_size_class(binding):
    """n = 1000 (no multiple of 8, 64 or 512).  1 x 1: every lane on one counter; 300 x 300 = 90000 cells: beyond the 16384 of LDS, straight
    into the global table; 300 x 33 and 33 x 300 fit the budget alone; the diagonals are the cluster sizes."""
    n, K = 1000, [1, 2, 7, 33, 300]
    rng = np.random.default_rng(0)
    ids = [rng.integers(0, k, n) for k in K]
    wk = worker(binding, n, ids, K)
    pairs = [(s, t) for s in range(5) for t in range(s, 5)]
    assert len(pairs) == 15
    got = wk.trace_tables(pairs)
    check_tables(got, pairs, ids, K)
    assert got[0].tolist() == [[n]] and np.array_equal(np.diag(got[-1]), np.bincount(ids[4], minlength=300)) and got[-1].sum() == n
    back = [(t, s) for s, t in pairs]
    for a, b in zip(wk.trace_tables(back), got):                     # the transposed pair is the transposed table
        assert np.array_equal(a, b.T)
    assert wk.trace_tables([]) == []
    wk.close()


def test_many_pairs_in_any_order_and_one_at_a_time(binding):
    """n = 70001, 12 slots of K = 40: 78 tables of 1600 cells = 124800 cells, a row's pairs split over groups, several workgroups per group."""
    n, T, K = 70001, 12, 40
    rng = np.random.default_rng(1)
    base = rng.integers(0, K, n)
    ids = [np.where(rng.random(n) < 0.3, rng.integers(0, K, n), (base + j) % K) for j in range(T)]
    wk = worker(binding, n, ids, [K] * T)
    pairs = [(s, t) for s in range(T) for t in range(s, T)]
    assert len(pairs) == 78
    got = wk.trace_tables(pairs)
    check_tables(got, pairs, ids, [K] * T)
    order = np.random.default_rng(2).permutation(len(pairs))
    shuffled = wk.trace_tables([pairs[i] for i in order])
    for i, t in zip(order, shuffled):
        assert np.array_equal(t, got[i])
    for i, p in enumerate(pairs):
        assert np.array_equal(wk.trace_tables([p])[0], got[i]), p
    wk.close()


def test_one_point_and_an_empty_shard(binding):
    wk = worker(binding, 1, [[2], [0]], [3, 1])
    a, b, d = wk.trace_tables([(0, 1), (1, 0), (0, 0)])
    assert a.tolist() == [[0], [0], [1]] and b.tolist() == [[0, 0, 1]] and d.tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, 1]]
    assert wk.trace_read(0).tolist() == [3] and wk.trace_read(1, device=DEV).tolist() == [1]
    assert wk.trace_confidence(0, [0, 1], [np.eye(3), np.ones((3, 1))]).tolist() == [1.0]
    wk.close()
    wk = worker(binding, 0, [[], []], [4, 5])
    got = wk.trace_tables([(0, 1), (1, 1)])
    assert [t.shape for t in got] == [(4, 5), (5, 5)] and not got[0].any() and not got[1].any()
    assert wk.trace_read(0).shape == (0,) and wk.trace_read(0, device=DEV).shape == (0,)
    assert wk.trace_confidence(0, [1], [np.zeros((4, 5))]).shape == (0,)
    assert wk.trace_confidence(0, [1], [np.zeros((4, 5))], device=DEV).shape == (0,)
    wk.close()


def test_overwrite_ignored_ids_and_refusals(binding):
    n = 777
    rng = np.random.default_rng(3)
    z0, z1, z2 = rng.integers(0, 5, n), rng.integers(0, 9, n), rng.integers(0, 5, n)
    wk = binding.Worker(binding.PRIOR_NIW, 2, n, device=0, seed=1)
    with pytest.raises(binding.DpmmError) as e:                       # no trace yet
        wk.trace_record(0, 5)
    assert e.value.code == ESTATE
    for slots in (0, -3, 4097):
        with pytest.raises(binding.DpmmError) as e:
            wk.trace_open(slots)
        assert e.value.code == EINVAL
    wk.trace_open(3)
    with pytest.raises(binding.DpmmError) as e:                       # no labels yet
        wk.trace_record(0, 5)
    assert e.value.code == ESTATE
    wk.set_labels(z0 + 1, np.ones(n, np.int64))
    for slot, K in ((3, 5), (-1, 5), (0, 0), (0, 1025)):
        with pytest.raises(binding.DpmmError) as e:
            wk.trace_record(slot, K)
        assert e.value.code == EINVAL, (slot, K)
    wk.trace_record(0, 5)
    wk._trace_K[1] = 9                                                 # (the binding sizes its buffer by what it recorded: pretend, the library refuses)
    with pytest.raises(binding.DpmmError) as e:                       # slot 1 was never recorded
        wk.trace_tables([(0, 1)])
    assert e.value.code == ESTATE
    with pytest.raises(binding.DpmmError) as e:
        wk.trace_read(1)
    assert e.value.code == ESTATE
    with pytest.raises(binding.DpmmError) as e:
        wk.trace_confidence(0, [1], [np.zeros((5, 9))])
    assert e.value.code == ESTATE
    wk._trace_K[7] = 5
    with pytest.raises(binding.DpmmError) as e:                       # slot 7 is outside the trace
        wk.trace_tables([(0, 7)])
    assert e.value.code == EINVAL
    # a slot recorded twice holds the later labels
    wk.set_labels(z1 + 1)
    wk.trace_record(1, 9)
    wk.set_labels(z2 + 1)
    wk.trace_record(0, 5)
    t01, t00 = wk.trace_tables([(0, 1), (0, 0)])
    assert np.array_equal(t01, want(z2, z1, 5, 9)) and np.array_equal(np.diag(t00), np.bincount(z2, minlength=5))
    # labels above the K stated for the slot are counted nowhere: z1 has ids up to 8, recorded as K = 6
    wk.set_labels(z1 + 1)
    wk.trace_record(2, 6)
    t20, t22 = wk.trace_tables([(2, 0), (2, 2)])
    assert np.array_equal(t20, want(z1, z2, 6, 5)) and t20.sum() == np.sum(z1 < 6) < n and np.array_equal(np.diag(t22), np.bincount(z1, minlength=9)[:6])
    # opening again replaces the trace: nothing is recorded any more
    wk.trace_open(2)
    wk._trace_K[0] = 5
    with pytest.raises(binding.DpmmError) as e:
        wk.trace_read(0)
    assert e.value.code == ESTATE
    wk.trace_close()
    wk.trace_close()
    with pytest.raises(binding.DpmmError) as e:
        wk.trace_record(0, 5)
    assert e.value.code == ESTATE
    wk.close()


def test_trace_read_round_trip(binding):
    n = 4099
    rng = np.random.default_rng(4)
    ids = [rng.integers(0, 1024, n), rng.integers(0, 3, n)]
    wk = worker(binding, n, ids, [1024, 3])
    for j in range(2):
        h, d = wk.trace_read(j), wk.trace_read(j, device=DEV)
        assert h.dtype == np.int64 and d.dtype == torch.int64 and d.device == torch.device(DEV)
        assert np.array_equal(h, ids[j] + 1) and np.array_equal(d.cpu().numpy(), ids[j] + 1)
    assert np.array_equal(wk.get_labels()[0], ids[1] + 1)            # reading the trace leaves the labels in force alone
    wk.close()


def test_confidence_against_float64_and_its_bits(binding, summary):
    n, T = 5003, 9
    K = [3, 5, 1, 17, 4, 40, 2, 6, 300, 5]                            # T samples and the anchor's slot T
    rng = np.random.default_rng(5)
    base = rng.integers(0, 300, n)
    ids = [np.where(rng.random(n) < 0.25, rng.integers(0, k, n), base % k) for k in K]
    wk = worker(binding, n, ids, K)
    pairs = summary.pair_list(T)
    tables = dict(zip(pairs, wk.trace_tables(pairs)))
    for anchor in (T, 3):
        ratio = summary.ratio_tables(tables, anchor, T)
        assert all(r.dtype == np.float32 and r.min() >= 0 and r.max() <= 1 for r in ratio)
        exact = np.zeros(n)
        for s in range(T):                                            # the share of the anchor's cluster of i that sits in i's cluster of sample s
            exact += want(ids[anchor], ids[s], K[anchor], K[s])[ids[anchor], ids[s]] / np.bincount(ids[anchor], minlength=K[anchor])[ids[anchor]]
        exact /= T
        h = wk.trace_confidence(anchor, list(range(T)), ratio)
        d = wk.trace_confidence(anchor, list(range(T)), ratio, device=DEV)
        assert h.dtype == np.float32 and d.dtype == torch.float32 and h.shape == (n,)
        err = np.abs(h.astype(np.float64) - exact).max()
        print(f"confidence, anchor {anchor}: max |error| = {err:.3e}, bound {(T + 2) * 2.0 ** -24:.3e}")
        assert err <= (T + 2) * 2.0 ** -24
        assert h.min() > 0 and h.max() <= 1
        assert np.array_equal(h.view(np.uint32), d.cpu().numpy().view(np.uint32))                       # host and device output: the same bits
        assert np.array_equal(h.view(np.uint32), wk.trace_confidence(anchor, list(range(T)), ratio).view(np.uint32))      # and again
        off = torch.empty(n + 1, dtype=torch.float32, device=DEV)[1:]      # an output that is not 16-byte aligned
        wk._chk(wk._lib.dpmm_trace_confidence(wk._h, anchor, np.arange(T, dtype=np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), T,
                                              np.concatenate([r.ravel() for r in ratio]).ctypes.data_as(binding._c_f32p), None,
                                              ctypes.c_void_p(off.data_ptr())))
        assert np.array_equal(h.view(np.uint32), off.cpu().numpy().view(np.uint32))
        assert np.array_equal(h.view(np.uint32), summary.confidence_numpy(ids[anchor], ids[:T], ratio).view(np.uint32))   # the numpy fallback: the same bits
    good = torch.empty(n + 8, dtype=torch.int64, device=DEV)
    host_memory = np.empty(n, np.int64)
    one, flat = np.zeros(1, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), np.zeros(9, np.float32).ctypes.data_as(binding._c_f32p)
    for ptr, word in ((host_memory.ctypes.data, "out_device"), (good.data_ptr() + 2, "aligned")):      # no device memory | misaligned for Float32
        with pytest.raises(binding.DpmmError) as e:
            wk._chk(wk._lib.dpmm_trace_confidence(wk._h, 0, one, 1, flat, None, ctypes.c_void_p(ptr)))
        assert e.value.code == EINVAL and word in str(e.value), str(e.value)
    for ptr, word in ((host_memory.ctypes.data, "labels_device"), (good.data_ptr() + 4, "aligned")):   # ... for Int64
        with pytest.raises(binding.DpmmError) as e:
            wk._chk(wk._lib.dpmm_trace_read(wk._h, 0, None, ctypes.c_void_p(ptr)))
        assert e.value.code == EINVAL and word in str(e.value), str(e.value)
    for call in (lambda: wk._lib.dpmm_trace_confidence(wk._h, 0, one, 1, flat, None, None), lambda: wk._lib.dpmm_trace_read(wk._h, 0, None, None)):
        with pytest.raises(binding.DpmmError) as e:                   # no output at all
            wk._chk(call())
        assert e.value.code == EINVAL
    wk.close()


def test_fit_on_a_device_tensor_end_to_end(host):
    """N = 4000, D = 2, four well-separated clusters.  The chain is bit-identical with and without the trace; the summary lives on the
    device, recomputes from its samples, and its estimate is no worse against the ground truth than the final labels (+ 0.02)."""
    N, T, iters = 4000, 8, 40
    x, y = host.generate_gaussian_data(N, 2, 4, 100.0, seed=6)[:2]
    y = np.asarray(y, np.int64)
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)
    kw = dict(iters=iters, seed=21, burnout=5, verbose=False)
    ref = host.fit(t, 10.0, **kw)
    got = host.fit(t, 10.0, keep_samples=T, **kw)
    assert ref[8].summary is None
    assert torch.equal(got[0], ref[0]) and torch.equal(got[7], ref[7]) and got[6] == ref[6]
    sm = got[8].summary
    assert sm.iterations == list(range(iters - 5 - T, iters - 5)) + [iters]
    for v, dt in ((sm.labels, torch.int64), (sm.confidence, torch.float32), (sm.sample(0), torch.int64)):
        assert isinstance(v, torch.Tensor) and v.device == torch.device(DEV) and v.dtype == dt and v.shape == (N,)
    check_summary_recomputes(sm, T, N, iters, got[8].labels)
    final = got[8].labels.cpu().numpy()

    def against_truth(lab):
        C = np.zeros((lab.max(), y.max()))
        np.add.at(C, (lab - 1, y - 1), 1)
        return vi_numpy(C), binder_numpy(lab, y)
    vi_f, b_f = against_truth(final)
    for loss in ("vi", "binder"):
        vi_c, b_c = against_truth(sm.choose(loss).labels.cpu().numpy())
        print(f"{loss}: chosen slot {sm.index}, VI {vi_c:.4f} (final {vi_f:.4f}), Binder {b_c:.4f} (final {b_f:.4f})")
        assert vi_c <= vi_f + 0.02 and b_c <= b_f + 0.02
