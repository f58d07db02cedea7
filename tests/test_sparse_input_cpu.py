"""Sparse (CSC) count data through the public entry points, on the CPU: the host side of the feature -- input forms, sharding,
canonicalisation, rejections -- over the oracle-backed stand-in worker (which has no sparse upload: the shard is made dense on the
host for it, so the chains must be the dense chains bit for bit)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _host():
    from __graft_entry__ import load_package
    load_package()
    return importlib.import_module("dpmmsubclusters_jl_amd.host")


def _dense_to_tuple(x):
    D, N = x.shape
    cols = [np.nonzero(x[:, i])[0] for i in range(N)]
    colptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    rv = np.concatenate(cols).astype(np.int64)
    nz = np.concatenate([x[c, i] for i, c in enumerate(cols)]).astype(np.float32)
    return colptr, rv, nz, (D, N)


def _fit(host, data, D, **kw):
    from fake_worker import FakeWorker
    hyper = host.multinomial_hyper(np.ones(D))
    res = host.fit(data, hyper, 10.0, iters=30, seed=17, burnout=5, verbose=False, worker_factory=FakeWorker, nthreads=1, **kw)
    return res[0], res[7], np.array(res[6])


def _chains_equal(host, x, forms):
    ref = _fit(host, x, x.shape[0])
    for name, data in forms.items():
        got = _fit(host, data, x.shape[0])
        for a, b in zip(ref, got):
            assert np.array_equal(a, b), name
    assert ref[2][-1] >= 2        # (the chain did something: clusters were split off)


def test_fit_takes_the_same_chain_for_the_tuple_form():
    host = _host()
    x, _, _ = host.generate_mnmm_data(2000, 60, 4, 80, seed=3)
    _chains_equal(host, x, dict(tuple=_dense_to_tuple(x)))


def test_fit_takes_the_same_chain_for_every_input_form():
    sp = pytest.importorskip("scipy.sparse")
    host = _host()
    x, _, _ = host.generate_mnmm_data(2000, 60, 4, 80, seed=3)
    _chains_equal(host, x, dict(csc=sp.csc_matrix(x), csr_T=sp.csr_matrix(np.ascontiguousarray(x.T)).T, tuple=_dense_to_tuple(x)))


def test_non_canonical_scipy_input_is_made_canonical_on_a_copy():
    sp = pytest.importorskip("scipy.sparse")
    host = _host()
    x, _, _ = host.generate_mnmm_data(300, 20, 3, 40, seed=4)
    m = sp.csc_matrix(x)
    # the same matrix with every column's entries reversed and one entry split in two (a duplicate index)
    indptr = m.indptr.copy()
    ind, dat = [], []
    for i in range(m.shape[1]):
        a, b = indptr[i], indptr[i + 1]
        ind.append(m.indices[a:b][::-1]); dat.append(m.data[a:b][::-1])
    messy = sp.csc_matrix((np.concatenate(dat), np.concatenate(ind), indptr), shape=m.shape)
    assert not messy.has_sorted_indices
    before = messy.indices.copy()
    csc = importlib.import_module("dpmmsubclusters_jl_amd.host.sparse").as_csc(messy)
    assert np.array_equal(messy.indices, before)                       # the caller's object is untouched
    assert np.array_equal(csc.dense_rows(0, 300), x.T)


def test_generate_mnmm_data_sparse_is_the_dense_return():
    host = _host()
    x, lab, cl = host.generate_mnmm_data(1500, 70, 5, 60, seed=9)
    (cp, rv, nz, shape), lab2, cl2 = host.generate_mnmm_data(1500, 70, 5, 60, seed=9, sparse=True)
    assert shape == (70, 1500) and np.array_equal(lab, lab2) and np.array_equal(cl, cl2)
    csc = importlib.import_module("dpmmsubclusters_jl_amd.host.sparse").CSC(cp, rv, nz, shape)
    assert np.array_equal(csc.dense_rows(0, 1500).T, x)
    assert (nz != 0).all() and cp[-1] == np.count_nonzero(x)
    csc.columns(0, 1500)                                               # canonical: passes the host check
    # a vocabulary wide enough that a cluster's points are drawn in several blocks (32 MB / (8 B x D) = 419 points): the same draws
    x, lab, _ = host.generate_mnmm_data(1300, 10000, 2, 30, seed=2)
    (cp, rv, nz, shape), lab2, _ = host.generate_mnmm_data(1300, 10000, 2, 30, seed=2, sparse=True)
    assert np.array_equal(lab, lab2)
    assert np.array_equal(importlib.import_module("dpmmsubclusters_jl_amd.host.sparse").CSC(cp, rv, nz, shape).dense_rows(0, 1300).T, x)


def test_rejections():
    host = _host()
    x, _, _ = host.generate_mnmm_data(200, 12, 3, 30, seed=1)
    cp, rv, nz, shape = _dense_to_tuple(x)
    with pytest.raises(TypeError):                                     # Gaussian prior (also the default prior of fit(all_data, alpha))
        host.fit((cp, rv, nz, shape), host.niw_hyperparams(1.0, np.zeros(12), 15, np.eye(12)), 10.0, iters=2, verbose=False)
    with pytest.raises(TypeError):
        host.fit((cp, rv, nz, shape), 10.0, iters=2, verbose=False)
    with pytest.raises(ValueError, match="prior dimension 13 != data dimension 12"):
        _fit(host, (cp, rv, nz, shape), 13)
    first = int(np.nonzero(np.diff(cp) >= 2)[0][0])                    # a point with two entries at least
    a = cp[first]
    unsorted = rv.copy(); unsorted[a], unsorted[a + 1] = rv[a + 1], rv[a]
    with pytest.raises(ValueError, match=f"point {first}: row indices are not strictly increasing"):
        _fit(host, (cp, unsorted, nz, shape), 12)
    dup = rv.copy(); dup[a + 1] = dup[a]
    with pytest.raises(ValueError, match=f"point {first}: row indices are not strictly increasing"):
        _fit(host, (cp, dup, nz, shape), 12)
    oob = rv.copy(); oob[cp[first + 1] - 1] = 12
    with pytest.raises(ValueError, match=f"point {first}: row index out of range"):
        _fit(host, (cp, oob, nz, shape), 12)
    dec = cp.copy(); dec[5] = dec[4] - 1 if dec[4] > 0 else dec[6] + 1
    with pytest.raises(ValueError, match="colptr decreases at point"):
        _fit(host, (dec, rv, nz, shape), 12)


def _topics(D, K, n, per_point, seed):
    """K well-separated topics over a vocabulary of D: topic k puts 90 % of its mass on its own block of min(400, D / K) words (uniform), the
    rest on the whole vocabulary; a point draws `per_point` tokens.  Built as CSC only (the dense array is never made)."""
    rng = np.random.default_rng(seed)
    z = rng.integers(0, K, n)
    own = rng.random((n, per_point)) < 0.9
    words = np.where(own, z[:, None] * (D // K) + rng.integers(0, min(400, D // K), (n, per_point)), rng.integers(0, D, (n, per_point)))
    words.sort(axis=1)
    first = np.ones_like(words, bool); first[:, 1:] = words[:, 1:] != words[:, :-1]
    counts = first.sum(1)
    colptr = np.zeros(n + 1, np.int64); np.cumsum(counts, out=colptr[1:])
    rv = words[first].astype(np.int64)
    start = np.flatnonzero(first.ravel())
    nz = np.diff(np.append(start, words.size)).astype(np.float32)      # run lengths = token counts (runs never cross a point: each row starts one)
    return (colptr, rv, nz, (D, n)), z + 1


def test_topic_recipe_is_recovered_on_the_cpu_at_small_vocabulary():
    """The recipe of the large-vocabulary GPU test (tests/test_gpu_mult_sparse.py) at D = 2048, dense, over the oracle-backed worker: the 8 topics are recovered on the schedule
    of the dense module test (iters=60, burnout=5), so the threshold asked of the GPU run is one the recipe meets."""
    host = _host()
    from fake_worker import FakeWorker
    sparse = importlib.import_module("dpmmsubclusters_jl_amd.host.sparse")
    data, y = _topics(2048, 8, 4000, 50, seed=2)
    x = sparse.as_csc(data).dense_rows(0, 4000).T
    res = host.fit(x, host.multinomial_hyper(np.ones(2048, np.float32)), 10.0, iters=60, burnout=5, gt=y, seed=5, verbose=False,
                   worker_factory=FakeWorker, nthreads=1)
    assert res[4][-1] > 0.9


# ---- world 2 over gloo, N odd: the same chain as world 1 (each rank uploads its own columns only)
def _run(rank, world, port, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    host = _host()
    from fake_worker import FakeWorker
    comm = None
    if world > 1:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from dpmmsubclusters_jl_amd.host.comm import TorchDistComm
        comm = TorchDistComm()
    data, _, _ = host.generate_mnmm_data(1501, 40, 3, 60, seed=6, sparse=True)
    res = host.fit(data, host.multinomial_hyper(np.ones(40)), 10.0, iters=30, seed=23, burnout=5, verbose=False, comm=comm,
                   worker_factory=FakeWorker, nthreads=1)
    if rank == 0:
        np.savez(out, labels=res[0], K=np.array(res[6]), sub=res[7])
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_match_one_rank_on_sparse_input(tmp_path):
    o1, o2 = str(tmp_path / "r1.npz"), str(tmp_path / "r2.npz")
    _run(0, 1, 0, o1)
    mp.spawn(_run, args=(2, 29641, o2), nprocs=2, join=True)
    a, b = np.load(o1), np.load(o2)
    for k in ("labels", "K", "sub"):
        assert np.array_equal(a[k], b[k]), k
