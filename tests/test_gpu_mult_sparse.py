"""GPU tests of the sparse (CSC) point storage of the Multinomial prior (dpmm_upload_points_csc, csrc/mult_sparse.hip).
Tolerances are those of tests/test_gpu_mult.py for the same quantities: table rtol 1e-5 / atol 1e-3 against the Float64 product,
draws bit-exact given the GPU's own table, counted near-boundary flips against the oracle and the dense worker, statistics of
count data exact."""
import importlib

import numpy as np
import pytest

from oracle import oracle as orc
from test_gpu_mult import make_problem
from test_sparse_input_cpu import _topics

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def host(pkg):
    return importlib.import_module("dpmmsubclusters_jl_amd.host")


def to_csc(X):
    """(n, D) rows -> colptr, rowval, nzval of the D x n matrix (one column per point), canonical, 0-based."""
    r, c = np.nonzero(X)
    colptr = np.zeros(X.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=X.shape[0]), out=colptr[1:])
    return colptr, c.astype(np.int64), X[r, c].astype(np.float32)


def sparse_worker(pkg, P, seed, first=0, params=True):
    wk = pkg.Worker(pkg.PRIOR_MULT, P["D"], P["n"], first_index=first, device=0, seed=seed)
    wk.upload_points_csc(*to_csc(P["X"]))
    if params:
        wk.set_params_mult(P["logp"], P["lr"], P["w"])
    return wk


def dense_worker(pkg, P, seed, first=0):
    wk = pkg.Worker(pkg.PRIOR_MULT, P["D"], P["n"], first_index=first, device=0, seed=seed)
    wk.upload_points(P["X"])
    wk.set_params_mult(P["logp"], P["lr"], P["w"])
    return wk


def _special(D, n, K, trials, seed):
    """make_problem's recipe with empty columns and one column that holds all D features."""
    P = make_problem(D, n, K, trials, seed)
    P["X"][::5] = 0.0
    P["X"][3] = 1.0 + (np.arange(D) % 3)
    return P


CASES = [(100, 1000, 2, 50), (1000, 3000, 32, 100), (37, 2049, 7, 20), (257, 1500, 50, 60), (20000, 4000, 12, 150)]


@pytest.mark.parametrize("D,n,K,trials", CASES + [(300, 1111, 6, 40)])
def test_table_labels_and_dense_parity(pkg, D, n, K, trials):
    P = _special(D, n, K, trials, seed=1) if D == 300 else make_problem(D, n, K, trials, seed=D + K)
    seed, epoch, first = 99, 3, 12345
    wk = sparse_worker(pkg, P, seed, first)
    tab = wk.debug_loglik()
    want = np.stack([P["X"].astype(np.float64) @ P["logp"][3 * k].astype(np.float64) + np.log(np.float64(P["w"][k])) for k in range(K)])
    np.testing.assert_allclose(tab, want, rtol=1e-5, atol=1e-3)
    wk.sweep(epoch)
    lab, sub = wk.get_labels()
    u0, u1 = orc.uniforms(seed, epoch, 0, first, n)
    assert np.array_equal(orc.sample_log_cat(tab, u0), lab)
    tab2 = wk.debug_subloglik()
    i = np.arange(n)
    pair = np.stack([tab2[2 * (lab - 1), i], tab2[2 * (lab - 1) + 1, i]])
    assert np.array_equal(orc.sample_log_cat(pair, u1), sub)
    olab, osub = orc.sweep_mult(P["X"], D, P["logp"], np.log(P["w"]), np.log(P["lr"]), seed, epoch, first)
    same = lab == olab
    dk = dense_worker(pkg, P, seed, first)
    dk.sweep(epoch)
    dlab, dsub = dk.get_labels()
    dk.close()
    dsame = lab == dlab
    print(f"sparse D={D} K={K} n={n}: label flips vs oracle {(lab != olab).sum()}, sub-label flips {(sub[same] != osub[same]).sum()}; "
          f"vs dense worker {(lab != dlab).sum()}, {(sub[dsame] != dsub[dsame]).sum()}")
    assert (lab != olab).sum() <= max(1, int(1e-5 * n))
    assert (sub[same] != osub[same]).sum() <= max(2, int(1e-4 * n))
    assert (lab != dlab).sum() <= max(1, int(1e-5 * n))
    assert (sub[dsame] != dsub[dsame]).sum() <= max(2, int(1e-4 * n))
    wk.sweep(epoch + 1, final=True)
    assert np.array_equal(wk.get_labels()[0], orc.argmax_rows(tab))
    wk.close()


def test_empty_shard(pkg):
    wk = pkg.Worker(pkg.PRIOR_MULT, 50, 0, device=0, seed=1)
    wk.upload_points_csc(np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32))
    P = make_problem(50, 10, 3, 10, seed=2)
    wk.set_params_mult(P["logp"], P["lr"], P["w"])
    wk.init_labels(3, 1)
    wk.sweep(1)
    st = wk.suffstats_packed()
    assert st.shape == (6, 51) and not st.any()
    wk.close()


@pytest.mark.parametrize("D,n,K", [(1000, 20000, 32), (100, 5000, 3), (7, 3000, 4), (40, 6000, 600)])
def test_suffstats_equal_dense_and_oracle(pkg, D, n, K):
    rng = np.random.default_rng(D)
    X = rng.poisson(0.3, size=(n, D)).astype(np.float32)
    lab = rng.integers(1, K + 1, n); sub = rng.integers(1, 3, n)
    out = {}
    for kind in ("sparse", "dense"):
        wk = pkg.Worker(pkg.PRIOR_MULT, D, n, device=0, seed=1)
        wk.upload_points_csc(*to_csc(X)) if kind == "sparse" else wk.upload_points(X)
        wk.set_labels(lab, sub)
        wk.set_num_clusters(K)
        out[kind] = (wk.suffstats(), wk.suffstats(np.array([1, K])))
        wk.close()
    oN, os_ = orc.suffstats_mult(X, D, lab, sub, K)
    N, s = out["sparse"][0]
    assert np.array_equal(N, oN.astype(np.float64)) and np.array_equal(s, os_.astype(np.float64))
    for a, b in zip(out["sparse"][0] + out["sparse"][1], out["dense"][0] + out["dense"][1]):
        assert np.array_equal(a, b)
    assert out["sparse"][1][0][0, 0] == (lab == 1).sum() and (out["sparse"][1][0][1:K - 1] == 0).all()


def test_suffstats_of_non_integer_values_are_deterministic(pkg):
    D, n, K = 120, 7000, 5
    rng = np.random.default_rng(8)
    X = rng.poisson(0.4, size=(n, D)).astype(np.float32)
    X = np.where(X > 0, X + np.float32(0.3), 0).astype(np.float32)
    lab = rng.integers(1, K + 1, n); sub = rng.integers(1, 3, n)
    wk = pkg.Worker(pkg.PRIOR_MULT, D, n, device=0, seed=1)
    wk.upload_points_csc(*to_csc(X))
    wk.set_labels(lab, sub)
    wk.set_num_clusters(K)
    a = wk.suffstats_packed(); b = wk.suffstats_packed()
    assert np.array_equal(a, b)
    want = np.zeros((2 * K, 1 + D))
    np.add.at(want, 2 * (lab - 1) + (sub - 1), np.concatenate([np.ones((n, 1)), X.astype(np.float64)], axis=1))
    np.testing.assert_allclose(a, want, rtol=1e-12)
    wk.close()


def test_suffstats_golden_bit_exact_through_the_sparse_path(pkg, golden_dir):
    g = np.load(f"{golden_dir}/mnm_golden.npz")
    X = np.ascontiguousarray(g["X"], np.float32)
    wk = pkg.Worker(pkg.PRIOR_MULT, 100, 1000, device=0, seed=1)
    wk.upload_points_csc(*to_csc(X))
    wk.set_labels(g["labels"], g["sub"])
    wk.set_num_clusters(2)
    N, s = wk.suffstats()
    i = 0
    for k in range(2):
        for w in range(3):
            assert np.array_equal(s[k, w].astype(np.float32), g["points_sum"][i])
            assert np.array_equal((g["prior_alpha"] + s[k, w].astype(np.float32)).astype(np.float32), g["post_alpha"][i])
            i += 1
    assert N[:, 0].tolist() == [463, 537]
    wk.close()


def test_uploads_of_either_kind_follow_each_other(pkg):
    """Parameters and labels survive an upload of the other kind of data (the contract test_gpu_mult shows for dense uploads)."""
    P = make_problem(130, 2000, 6, 40, seed=4)
    Q = make_problem(130, 2000, 6, 40, seed=5)
    wk = dense_worker(pkg, P, seed=3)
    t_dense_P = wk.debug_loglik()
    wk.upload_points_csc(*to_csc(Q["X"]))
    t_sparse_Q = wk.debug_loglik()
    wk.upload_points(Q["X"])
    t_dense_Q = wk.debug_loglik()
    wk.upload_points_csc(*to_csc(P["X"]))
    t_sparse_P = wk.debug_loglik()
    np.testing.assert_allclose(t_sparse_Q, t_dense_Q, rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(t_sparse_P, t_dense_P, rtol=1e-5, atol=1e-3)
    assert not np.allclose(t_sparse_P, t_sparse_Q)
    wk.close()


def test_refused_uploads_leave_the_points_in_force(pkg):
    P = make_problem(60, 500, 3, 30, seed=6)
    wk = sparse_worker(pkg, P, seed=1)
    before = wk.debug_loglik()
    cp, rv, nz = to_csc(P["X"])
    first = int(np.nonzero(np.diff(cp) >= 2)[0][0]); a = cp[first]
    unsorted = rv.copy(); unsorted[a], unsorted[a + 1] = rv[a + 1], rv[a]
    dup = rv.copy(); dup[a + 1] = dup[a]
    oob = rv.copy(); oob[a] = 60
    for bad, what in ((unsorted, "strictly increasing"), (dup, "strictly increasing"), (oob, "out of range")):
        with pytest.raises(pkg.DpmmError, match=f"point {first}: .*{what}") as ei:
            wk.upload_points_csc(cp, bad, nz)
        assert ei.value.code == -1
        assert np.array_equal(wk.debug_loglik(), before)
    dec = cp.copy(); dec[7] = dec[6] - 1 if dec[6] > 0 else dec[8] + 1
    with pytest.raises(pkg.DpmmError, match="colptr decreases"):
        wk.upload_points_csc(dec, rv, nz)
    # 1-based input (Julia's SparseMatrixCSC) is the same points
    wk.upload_points_csc(cp + 1, rv + 1, nz, index_base=1)
    assert np.array_equal(wk.debug_loglik(), before)
    wk.close()
    niw = pkg.Worker(pkg.PRIOR_NIW, 4, 10, device=0, seed=1)
    with pytest.raises(pkg.DpmmError) as ei:
        niw.upload_points_csc(np.zeros(11, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32))
    assert ei.value.code == -1
    niw.close()
    big = pkg.Worker(pkg.PRIOR_MULT, 65537, 10, device=0, seed=1)
    with pytest.raises(pkg.DpmmError) as ei:
        big.upload_points_csc(np.zeros(11, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32))
    assert ei.value.code == -5
    big.close()


def test_minus_inf_at_a_feature_a_point_does_not_store(pkg):
    """The stated deviation: 0 * log 0 = 0 for sparse points (an absent feature contributes nothing); the dense kernels follow IEEE."""
    P = make_problem(64, 600, 3, 20, seed=9)
    P["X"][:, 5] = 0.0
    P["X"][::2, 5] = 1.0                              # odd points do not store feature 5
    P["logp"][3, 5] = -np.inf                          # cluster 2's row
    sk, dk = sparse_worker(pkg, P, 1), dense_worker(pkg, P, 1)
    ts, td = sk.debug_loglik(), dk.debug_loglik()
    odd = np.arange(600) % 2 == 1
    assert np.isfinite(ts[1, odd]).all() and np.isneginf(ts[1, ~odd]).all()
    td = np.where(np.isnan(td), -np.inf, td)           # (nan_to_ninf, as the draw applies it)
    assert np.isneginf(td[1]).all()
    assert np.isfinite(ts[[0, 2]]).all()
    sk.close(); dk.close()


def _nmi_chain(pkg, host, data, y, D, N, dev, iters=60):
    engine = importlib.import_module("dpmmsubclusters_jl_amd.host.engine")
    hyper = host.multinomial_hyper(np.ones(D, np.float32))
    wk = pkg.Worker(hyper.kind, D, N, device=0, seed=5, timing=False)
    wk.upload_points_csc(data[0], data[1], data[2])
    s = host.DPMMSampler(wk, hyper, 10.0, N, 5, burnout=5)
    s.model.set_option(engine.OPT_DEVICE_MASTER, dev)
    s.init_first_clusters(1)
    _, nmi, _, kh = s.run_model(iters, 1, verbose=False, gt=y)
    wk.close()
    return nmi[-1], kh[-1]


def test_whole_chains_on_sparse_input(pkg, host):
    data, labels, _ = host.generate_mnmm_data(20000, 50, 5, 200, seed=3, sparse=True)
    res = host.fit(data, host.multinomial_hyper(np.ones(50, np.float32)), 10.0, iters=60, burnout=5, gt=labels, seed=5, verbose=False)
    assert res[4][-1] > 0.9
    # the engine's master with the draws on the device, and on the host
    data, y, _ = host.generate_mnmm_data(20000, 200, 5, 150, seed=3, sparse=True)
    for dev in (1, 0):
        nmi, K = _nmi_chain(pkg, host, data, y, 200, 20000, dev)
        print(f"sparse chain, device master {dev}: NMI {nmi:.4f}, K {K}")
        assert nmi > 0.9
    # predict: sparse against dense on the same points
    x, _, _ = host.generate_mnmm_data(20000, 50, 5, 200, seed=3)
    ls, ps = host.predict(res[8], host.generate_mnmm_data(20000, 50, 5, 200, seed=3, sparse=True)[0])
    ld, pd = host.predict(res[8], x)
    top2 = np.sort(pd, axis=1)[:, -2:]
    close = (top2[:, 1] - top2[:, 0]) < 1e-5
    print(f"predict: points with the top two probabilities within 1e-5: {close.mean():.2e}")
    assert close.mean() <= 1e-4
    assert np.array_equal(ls[~close], ld[~close])
    np.testing.assert_allclose(ps, pd, atol=1e-4)


def test_large_vocabulary_stays_sparse_on_the_device(pkg, host):
    """D = 65536, n = 200 000, 50 tokens per point: 52 GB as dense Float32.  The device may grow by an eighth of that at most."""
    import torch
    D, n, K = 65536, 200000, 8
    data, y = _topics(D, K, n, 50, seed=2)
    free0 = torch.cuda.mem_get_info(0)[0]
    hyper = host.multinomial_hyper(np.ones(D, np.float32))
    wk = pkg.Worker(hyper.kind, D, n, device=0, seed=5, timing=False)
    wk.upload_points_csc(data[0], data[1], data[2])
    s = host.DPMMSampler(wk, hyper, 10.0, n, 5, burnout=5)
    s.init_first_clusters(1)
    s.group_step(False, False)
    grown = free0 - torch.cuda.mem_get_info(0)[0]
    print(f"device memory growth after the first step: {grown / 2 ** 20:.0f} MiB (bound {D * n * 4 / 8 / 2 ** 20:.0f} MiB)")
    assert grown < D * n * 4 / 8
    wk.close()
    res = host.fit(data, hyper, 10.0, iters=60, burnout=5, gt=y, seed=5, verbose=False)
    print(f"large vocabulary: NMI {res[4][-1]:.4f}, K history tail {res[6][-5:]}")
    assert res[4][-1] > 0.9


# ---- a sparse fit saved and resumed with sparse data continues the chain (checkpoints and get_labels_histogram hold no points: nothing
# in them knows how the points were stored, so this is tests/test_gpu_checkpoint.py's dense test on the other upload)
def test_sparse_fit_saved_and_resumed_with_sparse_data(host, tmp_path):
    data, y, _ = host.generate_mnmm_data(6000, 80, 4, 120, seed=14, sparse=True)
    hyper = host.multinomial_hyper(np.ones(80, np.float32))
    r = host.fit(data, hyper, 10.0, iters=14, seed=5, burnout=4, verbose=False, save_model=True, save_path=str(tmp_path) + "/",
                 model_save_interval=7)
    model = r[8]
    assert len(model.checkpoints) == 2 and max(r[6]) > 1
    res, *_ = host.resume_from_checkpoint(model.checkpoints[0], data, 14, verbose=False)
    assert np.array_equal(res.labels, r[0]) and np.array_equal(res.labels_subcluster, model.labels_subcluster)
    assert res.sampler.K == model.sampler.K and np.array_equal(res.sampler.weights, model.sampler.weights)
    assert host.get_labels_histogram(res.labels) == host.get_labels_histogram(r[0])


# ---- LDS and registers poisoned (tests/test_gpu_uninit.py's method): the sparse sweep and statistics pass read nothing they did not write
@pytest.mark.parametrize("pattern", [0xffffffff, 0x7fc00000])
def test_sparse_sweep_and_statistics_ignore_lds_and_register_contents(pkg, pattern):
    import contextlib
    from tools import poison
    try:
        poison.build()
    except Exception as e:  # noqa: BLE001 -- test infrastructure, as in tests/test_gpu_uninit.py
        pytest.skip(f"tests/tools/libpoison.so cannot be built here: {e}")
    binding = importlib.import_module(pkg.__name__ + ".binding")
    P = _special(300, 5000, 40, 40, seed=21)                  # K > 32, empty columns, one full column; two sweeps: the scratch is reused
    P["X"][7] += np.float32(0.3)                              # (a non-integer column: the statistics are not exact sums by luck)
    out = []
    for dirty in (False, True, "kernels"):
        with (poison.poisoned_kernel_launches(binding, pattern) if dirty == "kernels" else contextlib.nullcontext()):
            wk = sparse_worker(pkg, P, seed=17, first=11)
            got = []
            for epoch in (1, 2):
                if dirty: poison.poison(pattern)
                wk.sweep(epoch)
                got += [np.array(a).copy() for a in wk.get_labels()]
                if dirty: poison.poison(pattern)
                got.append(wk.suffstats_packed().copy())
                if dirty: poison.poison(pattern)
                got.append(wk.suffstats_packed(np.array([2, 5])).copy())
            if dirty: poison.poison(pattern)
            got.append(wk.debug_loglik().copy())
            wk.close()
            out.append(got)
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)
    assert np.isfinite(out[0][2]).all() and len(np.unique(out[0][0])) > 1


# ---- worlds 2 and 3 over the host transport (all ranks on one GPU, as tests/test_gpu_multirank.py): every rank uploads its own columns
# -- a SLICE of colptr with colptr[0] != 0 and the entries it spans -- and the chain is the one-rank chain
def _rank(rank, world, port, out):
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from __graft_entry__ import load_package
    load_package()
    host = importlib.import_module("dpmmsubclusters_jl_amd.host")
    comm = None
    if world > 1:
        import torch.distributed as dist
        from dpmmsubclusters_jl_amd.host.comm import TorchDistComm
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        comm = TorchDistComm(device=0)
    N, D = 60001, 100                                         # N % 2 and N % 3 are not zero
    data, y, _ = host.generate_mnmm_data(N, D, 6, 80, seed=4242, sparse=True)
    res = host.fit(data, host.multinomial_hyper(np.ones(D, np.float32)), 10.0, iters=50, burnout=6, gt=y, seed=99, verbose=False,
                   comm=comm, device=0)
    info = res[8].sampler.wk.comm_info()
    if rank == 0:
        np.savez(out, labels=res[0], sub=res[7], K=np.array(res[6]), nmi=np.array(res[4], float), world=info["world"],
                 transport=str(info["transport"]))
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("world", [2, 3])
def test_ranks_on_sparse_shards_take_the_one_rank_chain(tmp_path, world):
    import torch.multiprocessing as mp
    o1, ow = str(tmp_path / "r1.npz"), str(tmp_path / "rw.npz")
    port = 29900 + 2 * world
    mp.spawn(_rank, args=(1, port, o1), nprocs=1, join=True)
    mp.spawn(_rank, args=(world, port + 1, ow), nprocs=world, join=True)
    a, b = np.load(o1), np.load(ow)
    assert int(b["world"]) == world and str(b["transport"]) == "host"
    assert np.array_equal(a["K"], b["K"]), (a["K"], b["K"])
    flips = int((a["labels"] != b["labels"]).sum())
    sflips = int(((a["sub"] != b["sub"]) & (a["labels"] == b["labels"])).sum())
    print(f"sparse shards, world {world}: K history equal (final {b['K'][-1]}), label flips {flips}, sub-label flips {sflips}, NMI {b['nmi'][-1]:.4f}")
    assert flips == 0 and sflips == 0
    assert b["K"][-1] >= 5 and b["nmi"][-1] > 0.9
