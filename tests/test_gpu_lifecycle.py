"""Who owns the memory of a context (csrc/dev_mem.h, csrc/dpmm_api.cpp): a context that used every kind of buffer gives all of it back,
growth of the device master's storage keeps the posterior state, and growth of the pinned statistics block changes no row."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_BIG = 9          # crosses the first cluster capacity (8)


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def hardware_queues_open():
    """The HIP runtime opens a hardware queue, with device memory of its own, the first time a stream is mapped to it, up to a handful per
    process.  A context brings two streams, so without this the SECOND context of a process opened two more queues: measured, 136 MiB
    less free memory after cycle 2 than after cycle 1 and not a byte more from then on, with the library of the parent commit as well.
    Eight streams that each ran a kernel leave nothing of that kind to the cycles (measured: five equal readings)."""
    import torch
    streams = [torch.cuda.Stream(device=0) for _ in range(8)]
    for s in streams:
        with torch.cuda.stream(s):
            torch.zeros(8, device="cuda:0").add_(1)
    torch.cuda.synchronize()


def _points(kind, D, n, rng):
    if kind == "niw":
        return (rng.normal(size=(n, D)) + 4.0 * rng.normal(size=(3, D))[rng.integers(0, 3, n)]).astype(np.float32)
    return rng.poisson(1.0, size=(n, D)).astype(np.float32)       # integer counts 0..255: the byte path


def _csc(X):
    rows = [np.nonzero(x)[0] for x in X]
    colptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return colptr, np.concatenate(rows).astype(np.int64), np.concatenate([x[r] for x, r in zip(X, rows)]).astype(np.float32)


def _cycle(pkg, kind, D, n):
    """create, upload, Gibbs steps with the device master, parameters for K_BIG clusters, one call of every feature, destroy"""
    import torch
    rng = np.random.default_rng(11)
    dev = torch.device("cuda:0")
    niw = kind == "niw"
    X = _points(kind, D, n, rng)
    wk = pkg.Worker(pkg.PRIOR_NIW if niw else pkg.PRIOR_MULT, D, n, device=0, seed=3, timing=False)
    if kind == "mult_csc":
        wk.upload_points_csc(*_csc(X))
    else:
        wk.upload_points(X)
    K = 2
    lr = np.full((K, 2), 0.5, np.float32); w = np.full(K, 1.0 / K, np.float32)
    slots = np.arange(K, dtype=np.int32)
    wk.init_labels(K, 0)
    wk.set_num_clusters(K)
    if niw:
        wk.master_setup(1.0, D + 3.0, np.zeros(D), np.eye(D))
    else:
        wk.mult_master_setup(np.ones(D, np.float32))
    for ep in range(1, 5):
        if niw:
            wk.step_master_device(ep, slots, draw_epoch=ep)
            wk.master_draw(ep, slots, lr, w)
        else:
            wk.step_stats(ep)
            wk.mult_master_draw(ep, lr, w)
        wk.sweep(ep)
    K = K_BIG
    lr = np.full((K, 2), 0.5, np.float32); w = np.full(K, 1.0 / K, np.float32)
    if niw:
        mu = rng.normal(size=(3 * K, D)).astype(np.float32)
        R = np.tile(np.eye(D, dtype=np.float32), (3 * K, 1, 1))
        wk.set_params_niw_chol(mu, R, np.zeros(3 * K, np.float32), lr, w)
        wk.set_predictive_niw(mu[0::3], R[0::3], np.zeros(K, np.float32), np.full(K, 5.0, np.float32), w)
    else:
        p = rng.dirichlet(np.ones(D), size=3 * K)
        wk.set_params_mult(np.log(p), lr, w)
        wk.set_predictive_mult(np.log(p[0::3]), w)
    assert wk.K == K
    wk.score_points(labels=True, logdens=True, probs=True)
    wk.score_points(labels=True, logdens=True, m=2, device=dev)
    wk.rank_begin(3); wk.rank_accumulate(0, n); wk.rank_read()
    wk.overlap_begin(); wk.overlap_accumulate(n); wk.overlap_read()
    wk.trace_open(2); wk.trace_record(0, K); wk.trace_record(1, K)
    wk.trace_tables([(0, 1)])
    wk.trace_confidence(0, [1], [np.ones((K, K), np.float32)])
    x = torch.empty((n, D), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    cstart = np.linspace(0, n, K + 1).astype(np.int64)
    if niw:
        wk.set_sampler_niw(mu[0::3], R[0::3], np.full(K, 5.0, np.float32))
        wk.sample_points_raw(0, n, cstart, 7, x=x.data_ptr(), ld=D)
        Xm = X.copy(); Xm[::7, 1] = np.nan
        wk.upload_points(Xm)
        out = np.empty((n, D), np.float32)
        wk.impute_points_into(out)
        assert np.isfinite(out).all()
        wk.set_projection(rng.normal(size=(D + 24, D)) / np.sqrt(D + 24), None)
        wk.upload_points_projected(rng.normal(size=(n, D + 24)).astype(np.float32))
    else:
        wk.set_sampler_mult(np.full((K, D), 2 ** 31, np.uint32), np.tile(np.arange(D, dtype=np.int32)[::-1], (K, 1)))
        wk.sample_points_raw(0, n, cstart, 7, trials=10, x=x.data_ptr(), ld=D)
    wk.close()
    del x
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


@pytest.mark.parametrize("kind,D,n", [("niw", 40, 4096), ("niw", 128, 2048), ("mult_dense", 32, 2048), ("mult_csc", 32, 2048)])
def test_cycle_returns_its_memory(pkg, hardware_queues_open, kind, D, n):
    """Three cycles: the free device memory after the second and third is the one after the first (which loaded the code objects and
    filled torch's cache).
    Measured on an MI355X, free bytes after cycles 1, 2, 3, this library | the library of the commit before the owners existed:
      niw 40 x 4096        308184875008 x 3                              | the same three
      niw 128 x 2048       308184875008 x 3                              | the same three
      mult_dense 32 x 2048 308180680704, 308180680704, 308178583552      | 308178583552, 308180680704, 308180680704
      mult_csc 32 x 2048   (not reached in that run)                     | 308178583552 x 3
    The dense Multinomial case moves by one 2 MiB block of the runtime's device heap, in either direction and with either library; five
    more cycles of a case add nothing.  No buffer of the library is behind it (every one is a member freed by dpmm_destroy); the
    assertion stays exact, as it was asked for, so this case can fail on that block."""
    free = [_cycle(pkg, kind, D, n) for _ in range(3)]
    print(f"{kind} D={D} n={n}: free device memory after each cycle {free}")
    assert free[1] == free[0] and free[2] == free[0], free


def _put_rows(wk, rows, K):
    rows = np.ascontiguousarray(rows, np.float64)
    wk._chk(wk._lib.dpmm_niw_master_put_rows(wk._h, rows.ctypes.data, int(K)))


def test_master_growth_keeps_the_posterior_state(pkg):
    """Slots 0, 1 get their posteriors while the master's storage holds 8 slots; posteriors for slots 8, 9 make it grow to 16 and must
    carry the state of slots 0, 1 over.  Against a context whose storage held 16 slots from the start: the stored rows of the four
    slots, and the labels of a sweep with parameters drawn from slots 0 and 9, bit for bit."""
    D, n, seed = 8, 2048, 5
    rng = np.random.default_rng(seed)
    X = _points("niw", D, n, rng)
    lab = rng.integers(1, 3, n); sub = rng.integers(1, 3, n)
    psi = np.eye(D) + 0.1
    stride = 1 + D + D * (D + 1) // 2
    rows = []
    for perm in (lab, 3 - lab):                   # two labellings with two clusters: their packed rows, from the library itself
        wk = pkg.Worker(pkg.PRIOR_NIW, D, n, device=0, seed=seed, timing=False)
        wk.upload_points(X); wk.set_labels(perm, sub); wk.set_num_clusters(2)
        rows.append(wk.suffstats_packed(None).copy())
        wk.close()
    assert rows[0].size == 4 * stride and not np.array_equal(rows[0], rows[1])

    def run(capacity_first):
        wk = pkg.Worker(pkg.PRIOR_NIW, D, n, device=0, seed=seed, timing=False)
        wk.upload_points(X); wk.set_labels(lab, sub)
        wk.master_setup(1.5, D + 3.0, np.full(D, 0.25), psi)
        if capacity_first:                        # one throw-away call with 16 clusters in 16 slots
            _put_rows(wk, np.zeros((32, stride)), 16)
            wk.master_posterior(None, np.arange(16, dtype=np.int32))
            wk.master_draw(9, np.arange(16, dtype=np.int32), np.full((16, 2), 0.5, np.float32), np.full(16, 1 / 16, np.float32))
        _put_rows(wk, rows[0], 2)
        wk.master_posterior(None, np.array([0, 1], np.int32))
        _put_rows(wk, rows[1], 2)
        wk.master_posterior(None, np.array([8, 9], np.int32))          # capacity 8 -> 16 where it was not forced
        stored = wk.master_rows(np.array([0, 1, 8, 9], np.int32))
        wk.master_draw(1, np.array([0, 9], np.int32), np.full((2, 2), 0.5, np.float32), np.full(2, 0.5, np.float32))
        draws = wk.master_draws(2)
        wk.sweep(2, final=True)
        labels = wk.get_labels()
        wk.close()
        return stored, draws, labels

    grown, forced = run(False), run(True)
    assert np.array_equal(grown[0][:2].reshape(4, stride), rows[0]) and np.array_equal(grown[0][2:].reshape(4, stride), rows[1])
    assert np.array_equal(grown[0], forced[0])
    for a, b in zip(grown[1], forced[1]):
        assert np.array_equal(a, b)
    assert np.array_equal(grown[2][0], forced[2][0]) and np.array_equal(grown[2][1], forced[2][1])


def test_pinned_statistics_block_grows_without_changing_a_row(pkg):
    """D = 128, K = 9: 2 * 9 * 8385 doubles, 1.2 MiB of packed rows, more than the first size of the pinned block (1 MiB).  The rows of a
    context whose block grew (it ran the same call with K = 2 first) against those of a fresh context, bit for bit."""
    D, n, K = 128, 2048, K_BIG
    rng = np.random.default_rng(8)
    X = _points("niw", D, n, rng)
    lab = 1 + np.arange(n) % K; sub = 1 + (np.arange(n) // K) % 2        # every sub-cluster populated: the pass resets nothing
    assert 2 * K * (1 + D + D * (D + 1) // 2) * 8 > 1 << 20

    def run(small_first):
        wk = pkg.Worker(pkg.PRIOR_NIW, D, n, device=0, seed=4, timing=False)
        wk.upload_points(X)
        if small_first:
            wk.set_labels(1 + np.arange(n) % 2, sub); wk.set_num_clusters(2)
            small, bad = wk.step_stats(1)
            assert small.shape[0] == 4 and not bad.any()
        wk.set_labels(lab, sub); wk.set_num_clusters(K)
        packed, bad = wk.step_stats(1)
        wk.close()
        return packed, bad

    grown, fresh = run(True), run(False)
    assert grown[0].shape == (2 * K, 1 + D + D * (D + 1) // 2)
    assert np.array_equal(grown[0][:, 0], np.bincount(2 * (lab - 1) + (sub - 1), minlength=2 * K))
    assert np.array_equal(grown[0], fresh[0]) and np.array_equal(grown[1], fresh[1])
