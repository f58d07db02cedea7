"""CPU-side checks of the posterior summary (include/dpmm_hip_trace.h, host/summary.py): the header compiles as C, its functions are bound,
exported and built from csrc/trace.hip; the two losses by hand; `fit(..., keep_samples=...)` over the oracle-backed stand-in leaves the
chain untouched and every field of `dp_model.summary` recomputes from `summary.sample(j)` with the numpy written here; shards add up;
the refusals.  The GPU counterparts are in test_gpu_summary.py."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package
from fake_worker import FakeWorker
from tools.summary_ref import check_summary_recomputes

HEADER = os.path.join(ROOT, "include", "dpmm_hip_trace.h")
TRACE_FUNCTIONS = ["dpmm_trace_close", "dpmm_trace_confidence", "dpmm_trace_open", "dpmm_trace_read", "dpmm_trace_record", "dpmm_trace_tables"]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def host(pkg):
    return importlib.import_module(pkg.__name__ + ".host")


@pytest.fixture(scope="module")
def summary(pkg):
    return importlib.import_module(pkg.__name__ + ".host.summary")


# ---------------------------------------------------------------------------------------------- the C boundary
def test_header_compiles_as_c_and_is_bound_exported_and_built(pkg):
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER])
    hdr = open(HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", body)))
    assert declared == TRACE_FUNCTIONS
    binding = importlib.import_module(pkg.__name__ + ".binding")
    assert sorted(n for n, _, _ in binding.ABI_TRACE) == declared
    others = binding.ABI + binding.ABI_TENSOR + binding.ABI_SCORE + binding.ABI_RANK + binding.ABI_MISSING + binding.ABI_CSC + binding.ABI_SAMPLE + binding.ABI_PROJECT
    assert not set(declared) & set(n for n, _, _ in others)
    protos = dict(re.findall(r"\b(dpmm_trace_[a-z]+)\s*\(([^;]*?)\)\s*;", body, flags=re.S))
    for name, _, args in binding.ABI_TRACE:                          # as many ctypes arguments as the prototype has parameters
        assert len(args) == protos[name].count(",") + 1, name
    for name in ("trace_open", "trace_close", "trace_record", "trace_tables", "trace_confidence", "trace_read"):
        assert callable(getattr(binding.Worker, name)), name
    assert int(re.search(r"#define DPMM_TRACE_MAX_SLOTS (\d+)", hdr).group(1)) == binding.TRACE_MAX_SLOTS == 4096
    mk = open(os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "build/trace.o" in objs and "dpmm_hip_trace.h" in mk
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for n in declared:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                               # additive: the version stays
    host = importlib.import_module(pkg.__name__ + ".host")
    assert host.PosteriorSummary is importlib.import_module(pkg.__name__ + ".host.summary").PosteriorSummary


# ---------------------------------------------------------------------------------------------- the losses
def test_losses_by_hand_renaming_and_the_tie_rule(summary):
    a = np.array([0, 0, 0, 1, 1, 1])
    b = np.array([0, 0, 1, 1, 2, 2])
    C = summary.contingency(a, b, 2, 3)
    assert C.dtype == np.int64 and C.tolist() == [[2, 1, 0], [0, 1, 2]]
    # Binder: n_a = (3, 3), n_b = (2, 2, 2), n_ab = (2, 1, 1, 2): (18 + 12 - 2 * 10) / 36
    assert summary.binder_from_contingency(C) == 10 / 36
    # ... which is the share of ordered pairs co-clustered in exactly one labelling, counted pair by pair
    assert summary.binder_from_contingency(C) == np.mean((a[:, None] == a[None, :]) != (b[:, None] == b[None, :]))
    # VI: H_a = ln 2, H_b = ln 3, I = 2 * (1/3) ln((1/3) / (1/6)) + 2 * (1/6) ln 1 = (2/3) ln 2
    tables = {(1, 0): C.T, (0, 0): np.diag([3, 3]), (1, 1): np.diag([2, 2, 2])}
    vi, binder = summary.loss_matrices(tables, 1)                    # one sample (a), candidates a and b
    assert vi.shape == binder.shape == (2, 1) and vi[0, 0] == 0.0 and binder[0, 0] == 0.0
    assert abs(vi[1, 0] - (np.log(3) - np.log(2) / 3)) < 1e-14 and binder[1, 0] == 10 / 36
    # an id at or above K of its side is counted nowhere
    assert summary.contingency(np.array([0, 1, 5]), np.array([1, 7, 0]), 2, 2).tolist() == [[0, 1], [0, 0]]
    # the same partition under other names: both losses are 0
    z = np.array([0, 0, 1, 2, 2, 1, 0])
    ren = np.array([2, 0, 1])[z]
    Cr = summary.contingency(z, ren, 3, 3)
    assert summary.binder_from_contingency(Cr) == 0.0
    t2 = {(1, 0): Cr.T, (2, 0): Cr.T, (2, 1): np.diag(np.bincount(ren)), (0, 0): np.diag(np.bincount(z)), (1, 1): np.diag(np.bincount(ren)),
          (2, 2): np.diag(np.bincount(ren))}
    vi2, b2 = summary.loss_matrices(t2, 2)
    assert np.all(b2 == 0.0) and np.all(np.abs(vi2) < 1e-15) and np.all(vi2 >= 0.0)
    # ties go to the lower slot: a sample beats the final labelling, an earlier sample a later one
    assert summary.select(b2.mean(1)) == 0
    assert summary.select([0.5, 0.25, 0.25]) == 1 and summary.select([0.25, 0.5, 0.25]) == 0
    # sums of squares leave Int64 for Python integers where they must: N = 2^33 points in one cell
    assert summary.binder_from_contingency(np.array([[2 ** 33, 0], [0, 2 ** 33]])) == 0.0
    assert summary.binder_from_contingency(np.array([[2 ** 33, 2 ** 33]])) == 0.5


# ---------------------------------------------------------------------------------------------- fit with keep_samples over the stand-in
class NoTraceWorker(FakeWorker):
    """A worker WITH the trace calls, every one of which refuses: without the keywords fit must not reach them."""
    def _refuse(self, *a, **k):
        raise AssertionError("a trace call without keep_samples")
    trace_open = trace_close = trace_record = trace_tables = trace_confidence = trace_read = _refuse


def test_fit_keeps_the_chain_and_every_field_recomputes(host, tmp_path):
    N, T, thin, iters = 900, 6, 2, 80
    rng = np.random.default_rng(1)                                   # two blobs that overlap (3.5 sigma apart) and one far from both
    y = np.arange(N) % 3
    x = (np.array([[0.0, 0.0], [3.5, 0.0], [12.0, 12.0]])[y] + rng.standard_normal((N, 2))).T.astype(np.float32)
    kw = dict(iters=iters, seed=31, burnout=4, verbose=False, nthreads=1, gt=y + 1)
    ref = host.fit(x, 10.0, worker_factory=NoTraceWorker, **kw)
    assert ref[8].summary is None
    got = host.fit(x, 10.0, worker_factory=FakeWorker, keep_samples=T, thin=thin, save_model=True, save_path=str(tmp_path) + "/",
                   model_save_interval=30, **kw)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[7], ref[7])                 # labels, sub-labels
    assert np.array_equal(got[8].labels, ref[8].labels) and np.array_equal(got[8].labels_subcluster, ref[8].labels_subcluster)
    assert got[4] == ref[4] and got[5] == ref[5] and got[6] == ref[6] and len(got[3]) == len(ref[3]) == iters      # the histories
    assert [os.path.basename(f) for f in got[8].checkpoints] == ["checkpoint__30.npz", "checkpoint__60.npz"]       # the other hook still runs
    sm = got[8].summary
    assert isinstance(sm, host.PosteriorSummary) and sm.loss == "vi" and sm.T == T
    i_end = iters - 5 - 1                                            # the last sweep that samples (argmax_sample_stop = 5)
    assert sm.iterations == [i_end - (T - 1 - j) * thin for j in range(T)] + [iters] == [64, 66, 68, 70, 72, 74, 80]
    assert isinstance(sm.labels, np.ndarray) and isinstance(sm.confidence, np.ndarray)
    z, stable = check_summary_recomputes(sm, T, N, iters, got[8].labels)
    assert len(stable) >= 1                                          # (the far blob: the check for a confidence of 1 was not empty)
    assert any(not np.array_equal(z[0], z[j]) for j in range(1, T))  # ... and the samples are not all the same labelling
    assert sm.confidence.min() < 0.9 and sm.expected_vi.min() > 0    # points between the two near blobs change partners
    with pytest.raises(IndexError):
        sm.sample(T + 1)
    with pytest.raises(ValueError, match="loss"):
        sm.choose("x")
    b = host.dp_parallel(x, host.niw_hyperparams(1.0, np.zeros(2), 5, np.eye(2)), 10.0, iters, 1, 31, False, burnout=4, nthreads=1,
                         worker_factory=FakeWorker, keep_samples=2, loss="binder")[0].summary
    assert b.loss == "binder" and b.index == int(np.argmin(b.expected_binder)) and b.iterations == [73, 74, 80]


def test_resume_from_checkpoint_records_its_part_of_the_chain(host, tmp_path):
    x, y = host.generate_gaussian_data(500, 2, 3, 60.0, seed=5)[:2]
    x = x.astype(np.float32)
    kw = dict(verbose=False, worker_factory=FakeWorker, nthreads=1)
    hyper = host.niw_hyperparams(1.0, np.zeros(2), 5, np.eye(2))
    full = host.dp_parallel(x, hyper, 10.0, 14, 2, seed=11, burnout=3, save_model=True, save_path=str(tmp_path) + "/", model_save_interval=4,
                            keep_samples=3, **kw)[0]
    res = host.resume_from_checkpoint(full.checkpoints[0], x, 14, keep_samples=3, **kw)[0]      # sweeps 5..14; recorded 6, 7, 8
    assert np.array_equal(res.labels, full.labels) and res.summary.iterations == full.summary.iterations == [6, 7, 8, 14]
    for j in range(4):
        assert np.array_equal(res.summary.sample(j), full.summary.sample(j))
    assert res.summary.index == full.summary.index and np.array_equal(res.summary.confidence, full.summary.confidence)
    with pytest.raises(ValueError, match="iters must be at least 16"):                           # first sweep 5: 5 + 5 + 1 + 5
        host.resume_from_checkpoint(full.checkpoints[0], x, 14, keep_samples=6, **kw)


# ---------------------------------------------------------------------------------------------- shards
def test_tables_of_two_shards_add_up_and_select_the_same(summary):
    rng = np.random.default_rng(3)
    N, T = 501, 4
    K = [3, 5, 4, 6, 5]
    base = rng.integers(0, 3, N)
    ids = [np.where(rng.random(N) < 0.2 * (j + 1), rng.integers(0, K[j], N), base % K[j]) for j in range(T + 1)]
    pairs = summary.pair_list(T)
    assert len(pairs) == T * (T + 1) // 2 + T + 1 and len(set(pairs)) == len(pairs)

    def tables(lo, hi):
        return {(s, t): summary.contingency(ids[s][lo:hi], ids[t][lo:hi], K[s], K[t]) for s, t in pairs}
    whole, a, b = tables(0, N), tables(0, 200), tables(200, N)
    for p in pairs:
        assert np.array_equal(a[p] + b[p], whole[p]) and whole[p].sum() == N, p
    summed = {p: a[p] + b[p] for p in pairs}
    for w, s in zip(summary.loss_matrices(whole, T), summary.loss_matrices(summed, T)):
        assert np.array_equal(w, s) and summary.select(w.mean(1)) == summary.select(s.mean(1))
    for anchor in (0, T):
        for rw, rs in zip(summary.ratio_tables(whole, anchor, T), summary.ratio_tables(summed, anchor, T)):
            assert rw.dtype == np.float32 and np.array_equal(rw, rs)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(host, tmp_path):
    x = np.random.default_rng(0).standard_normal((2, 50)).astype(np.float32)
    kw = dict(verbose=False, worker_factory=NoTraceWorker, nthreads=1, seed=1)
    with pytest.raises(ValueError, match="iters must be at least 17"):       # 1 + 5 + 1 + (6 - 1) * 2
        host.fit(x, 10.0, iters=16, keep_samples=6, thin=2, **kw)
    with pytest.raises(ValueError, match="loss"):
        host.fit(x, 10.0, iters=30, keep_samples=3, loss="x", **kw)
    for thin in (0, -1, 1.5):
        with pytest.raises(ValueError, match="thin"):
            host.fit(x, 10.0, iters=30, keep_samples=3, thin=thin, **kw)
    for T in (-1, 2.5, 4096):
        with pytest.raises(ValueError, match="keep_samples"):
            host.fit(x, 10.0, iters=30, keep_samples=T, **kw)
    f = tmp_path / "params.py"
    f.write_text("iterations = 3\n")
    with pytest.raises(TypeError, match="parameter file"):
        host.dp_parallel(str(f), keep_samples=3, **{k: kw[k] for k in ("verbose", "worker_factory", "nthreads")})
    with pytest.raises(TypeError):
        host.run_model_from_checkpoint(str(f), keep_samples=3)
