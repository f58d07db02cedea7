"""CPU-side checks of the count statistics (include/dpmm_hip_countstats.h) and of the Dirichlet update (host/absorb.py): the header
compiles as C, its functions are bound, exported and built from csrc/countstats.hip; `dirichlet_absorb` against its definition, the
Float64 survival of a small soft weight and its refusals; `Predictor.count_statistics` / `absorb_counts` over a stand-in worker that
keeps a numpy table: the slab walk, the NIW refusal, one reload of the predictives per absorb, the save / load round trip."""
import ctypes
import importlib
import os
import re
import subprocess
import types

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package
from tools import countstats_ref as C
from tools import overlap_ref, rank_ref
import test_rank_cpu as R

HEADER = os.path.join(ROOT, "include", "dpmm_hip_countstats.h")
FUNCS = ["dpmm_countstats_accumulate", "dpmm_countstats_begin", "dpmm_countstats_read"]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


@pytest.fixture(scope="module")
def host(pkg):
    return importlib.import_module(pkg.__name__ + ".host")


# ---------------------------------------------------------------------------------------------- the C boundary
def test_header_compiles_as_c_and_is_bound_exported_and_built(pkg, host, score):
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER])
    hdr = open(HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", body))) == FUNCS
    binding = importlib.import_module(pkg.__name__ + ".binding")
    assert sorted(n for n, _, _ in binding.ABI_COUNTSTATS) == FUNCS
    others = (binding.ABI + binding.ABI_TENSOR + binding.ABI_SCORE + binding.ABI_RANK + binding.ABI_OVERLAP + binding.ABI_BATCHSTATS + binding.ABI_TRACE
              + binding.ABI_MISSING + binding.ABI_IMPUTE + binding.ABI_CSC + binding.ABI_SAMPLE + binding.ABI_PROJECT)
    assert not set(FUNCS) & set(n for n, _, _ in others)
    for name in ("countstats_begin", "countstats_accumulate", "countstats_read", "countstats_read_raw"):
        assert callable(getattr(binding.Worker, name)), name
    assert eval(re.search(r"#define DPMM_COUNTSTATS_PARTIAL_BYTES \((\d+ << \d+)\)", hdr).group(1)) == binding.COUNTSTATS_PARTIAL_BYTES == 64 << 20
    struct = body[body.index("typedef struct {"):body.index("} dpmm_countstats_out;")]
    assert re.findall(r"\*\s*([A-Za-z_]+);", struct) == [f[0] for f in binding.CountStatsOut._fields_]
    assert re.findall(r"(double|int64_t)\s*\*", struct) == ["double"] * 2 + ["int64_t"] * 4
    csrc = os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "build/countstats.o" in re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "../../include/dpmm_hip_countstats.h" in re.search(r"^build/dpmm_api\.o:(.*)$", mk, flags=re.M).group(1).split()
    kern = open(os.path.join(csrc, "dpmm_kernels.h")).read()
    assert eval(re.search(r"COUNTSTATS_PARTIAL_BYTES = \(int64_t\)(\d+ << \d+);", kern).group(1)) == binding.COUNTSTATS_PARTIAL_BYTES
    hip = open(os.path.join(csrc, "countstats.hip")).read()
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in hip and '#include "score_device.h"' in hip and '#include "batchstats_device.h"' in hip
    assert not re.search(r"atomic\w*\(&?A\.(acc|part|npart)", hip)                  # the sums have one writer each: no atomics on them
    assert "dpmm_hip_countstats.h" in open(os.path.join(ROOT, "include", "dpmm_hip_batchstats.h")).read()      # the Limits paragraph points here
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for n in FUNCS:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                               # additive: the version stays
    for name in ("count_statistics", "dirichlet_absorb", "CountStatistics"):
        assert getattr(host, name) is getattr(score, name), name
    assert callable(host.Predictor.count_statistics) and callable(host.Predictor.absorb_counts)
    assert host.CountStatistics._fields == ("N", "sums", "count", "skipped", "incomplete", "held_out")


# ---------------------------------------------------------------------------------------------- the reference itself
def test_countstats_ref_on_points_written_by_hand():
    X = np.array([[1, 0, 2, np.nan, 5], [0, 3, 1, 1, 5]], np.float32)                    # (D = 2, n = 5)
    lab = np.array([1, 2, 1, 2, 2])
    P = np.array([[.75, .25], [.25, .75], [.5, .5], [.25, .75], [np.nan, np.nan]], np.float32)
    ld = np.array([-1, -2, -9, -1, 0], np.float32)
    h = C.stats(X, lab, P, "hard", ld, -5.0)
    assert (h["skipped"], h["held_out"], h["incomplete"]) == (1, 1, 1) and h["count"].tolist() == [1, 1]
    assert h["N"].tolist() == [1, 1] and h["sums"].tolist() == [[1, 0], [0, 3]]
    s = C.stats(X, lab, P, "soft")
    assert (s["skipped"], s["held_out"], s["incomplete"]) == (1, 0, 1) and s["count"].tolist() == [2, 1]
    assert s["N"].tolist() == [1.5, 1.5] and s["sums"].tolist() == [[.75 + 1, .75 + .5], [.25 + 1, 2.25 + .5]]
    import scipy.sparse as sp
    Xs = sp.csc_matrix(np.nan_to_num(X))
    hs = C.stats(Xs, lab, P, "hard")
    assert hs["sums"].tolist() == [[3, 1], [0, 4]] and hs["incomplete"] == 0
    N, sums = C.exact(Xs, lab, P)
    assert N.dtype == sums.dtype == np.int64 and sums.tolist() == [[3, 1], [0, 4]] and N.tolist() == [2, 2]
    assert C.within(dict(N=h["N"], sums=h["sums"] * (1 + 2.0 ** -52)), h, 5) <= 1 < C.within(dict(N=h["N"], sums=h["sums"] * (1 + 2.0 ** -40)), h, 5)


# ---------------------------------------------------------------------------------------------- dirichlet_absorb
def test_dirichlet_absorb_is_alpha_plus_sums_in_float64(host):
    rng = np.random.default_rng(1)
    K, D = 4, 6
    alpha = rng.gamma(2.0, 3.0, (K, D)).astype(np.float32)
    count = rng.integers(5, 50, K).astype(np.float64)
    N = np.array([3.0, 0.0, 2.5, 1.0])
    sums = rng.random((K, D)) * N[:, None]
    post = dict(alpha=alpha)
    new, cnt = host.dirichlet_absorb(post, count, types.SimpleNamespace(N=N, sums=sums))
    assert new["alpha"].dtype == np.float64 and post["alpha"] is alpha and alpha.dtype == np.float32      # the inputs are not modified
    want = alpha.astype(np.float64) + sums
    want[1] = alpha[1]                                                           # a cluster without weight keeps its values
    assert np.array_equal(new["alpha"], want) and np.array_equal(cnt, count + N)
    # conjugacy: two batches one after the other, or their union at once (Float64: to rounding)
    two, c2 = host.dirichlet_absorb(*host.dirichlet_absorb(post, count, dict(N=N, sums=sums)), dict(N=N[::-1], sums=sums[::-1]))
    one, c1 = host.dirichlet_absorb(post, count, dict(N=N + N[::-1], sums=sums + sums[::-1]))
    assert np.allclose(two["alpha"], one["alpha"], rtol=1e-15) and np.array_equal(c1, c2)
    # a soft weight of 0.01 on alpha = 1e6 survives in Float64; Float32, the type the reference keeps, would lose it
    big = dict(alpha=np.full((1, 2), 1e6, np.float32))
    small = dict(N=np.array([0.01]), sums=np.array([[0.01, 0.0]]))
    got = big
    c = np.array([1e6])
    for _ in range(100):
        got, c = host.dirichlet_absorb(got, c, small)
    assert abs(got["alpha"][0, 0] - (1e6 + 1.0)) < 1e-7 and got["alpha"][0, 1] == 1e6 and abs(c[0] - (1e6 + 1.0)) < 1e-7
    assert np.float32(1e6) + np.float32(0.01) == np.float32(1e6)
    f32 = host.multinomial_hyper(big["alpha"][0]).posterior(small["N"], small["sums"])["alpha"]
    assert f32.dtype == np.float32 and f32[0, 0] == np.float32(1e6)             # the fit's own update rounds it away


def test_dirichlet_absorb_refusals(host):
    post = dict(alpha=np.ones((2, 3), np.float32))
    count = np.array([4.0, 5.0])
    s = dict(N=np.array([1.0, 2.0]), sums=np.ones((2, 3)))
    for bad in (dict(s, N=s["N"][:1]), dict(s, sums=s["sums"][:, :2]), dict(s, N=np.array([1.0, -1.0])), dict(s, N=np.array([1.0, np.nan])),
                dict(s, N=np.array([np.inf, 1.0])), dict(s, sums=s["sums"] * np.nan), dict(s, sums=-s["sums"])):
        with pytest.raises(ValueError):
            host.dirichlet_absorb(post, count, bad)
    with pytest.raises(ValueError):
        host.dirichlet_absorb(post, count[:1], s)
    with pytest.raises(ValueError):
        host.dirichlet_absorb(dict(alpha=np.ones(3)), count, s)
    with pytest.raises(ValueError, match="Multinomial"):
        host.dirichlet_absorb(dict(kappa=np.ones(2), nu=np.ones(2), m=np.ones((2, 3)), U=np.ones((2, 3, 3))), count, s)


# ---------------------------------------------------------------------------------------------- Predictor.count_statistics / absorb_counts over a stand-in
class CountWorker(R.TableWorker):
    """tests/test_rank_cpu.py's table-keeping stand-in as a Multinomial worker, a_k(i) = log w_k + logp_k' x_i in Float32, with the calls
    `Predictor.count_statistics` makes, piece by piece through countstats_ref."""

    def set_predictive_mult(self, logp, weights):
        self.logp, self.logw, self.K = np.asarray(logp, np.float32), np.log(np.asarray(weights, np.float32)), len(weights)
        self.loads = getattr(self, "loads", 0) + 1
        self.cs_pieces = None                                                    # another parameter set: an accumulation does not survive it

    def table(self):
        with np.errstate(all="ignore"):
            return (self.logw[:, None] + self.logp @ self.X.T).astype(np.float32)     # (K, n)

    def scored(self, n_valid):
        tab = self.table()[:, :n_valid]
        P, lab, part = overlap_ref.probs(tab)
        P[~part] = np.nan                                                        # what `predict` writes for them
        _, M, _ = rank_ref.labels_and_scores(tab)
        with np.errstate(all="ignore"):
            ld = (M + np.log(np.exp(tab - M[None, :]).sum(0))).astype(np.float32)
        return self.X[:n_valid].T, lab, P, ld

    def countstats_begin(self, mode, min_logdens=None):
        self.cs_mode, self.cs_floor, self.cs_pieces, self.cs_calls = ("hard", "soft")[mode], min_logdens, [], []

    def countstats_accumulate(self, n_valid):
        assert 0 <= n_valid <= self.n and self.cs_pieces is not None
        self.cs_calls.append(int(n_valid))
        X, lab, P, ld = self.scored(n_valid)
        self.cs_pieces.append(C.stats(X, lab, P, self.cs_mode, ld, self.cs_floor))

    def countstats_read(self):
        r = C.add(self.cs_pieces) if self.cs_pieces else C.stats(np.zeros((self.D, 0), np.float32), np.zeros(0, np.int64), np.zeros((0, self.K), np.float32), "hard")
        return dict(r, **{f: np.array([r[f]], np.int64) for f in ("skipped", "incomplete", "held_out")})


N = 29
D, K = 5, 4


def alpha_post(seed=0):
    rng = np.random.default_rng(seed)
    a = 0.5 + rng.integers(0, 4, (K, D)).astype(np.float32)
    a[np.arange(K), np.arange(K)] += 8.0
    return dict(alpha=a)


def counts(n, seed):
    rng = np.random.default_rng(seed)
    return rng.poisson(1.5, (D, n)).astype(np.float32)


def open_mult(score, cap, factory=CountWorker, post=None, count=None):
    p = score.Predictor.__new__(score.Predictor)
    p._setup(1, D, 10.0, np.full(K, 20.0) if count is None else count, alpha_post() if post is None else post, cap, 0, factory)
    return p


def whole_reference(p, X, mode, floor=None):
    whole = CountWorker(1, X.shape[0], X.shape[1])
    whole.logp, whole.logw, whole.K = p._wk.logp, p._wk.logw, p._wk.K
    whole.upload_points(np.ascontiguousarray(X.T))
    Xs, lab, P, ld = whole.scored(X.shape[1])
    return C.stats(Xs, lab, P, mode, ld, floor), ld


@pytest.mark.parametrize("cap", [1, 7, N, N + 5])
@pytest.mark.parametrize("mode", ["hard", "soft"])
def test_predictor_count_statistics_walks_the_slabs(score, cap, mode):
    X = counts(N, 5)
    X[1, 11] = np.nan                                                            # a NaN row of the table: skipped
    with open_mult(score, cap) as p:
        wk = p._wk
        want, ld = whole_reference(p, X, mode)
        got = p.count_statistics(X, assign=mode)
        assert isinstance(got, score.CountStatistics) and all(isinstance(v, int) for v in got[3:]) and all(isinstance(a, np.ndarray) for a in got[:3])
        assert got.sums.shape == (K, D) and got.N.dtype == got.sums.dtype == np.float64 and got.count.dtype == np.int64
        assert wk.uploads == [cap] * -(-N // cap)                                 # never a short upload ...
        assert wk.cs_calls == [min(cap, N - lo) for lo in range(0, N, cap)]      # ... the padding is cut by n_valid
        assert C.within(got, want, N) <= 1 and np.array_equal(got.count, want["count"])
        assert (got.skipped, got.incomplete, got.held_out) == (1, 0, 0) and got.count.sum() == N - 1
        if mode == "hard":
            assert np.array_equal(got.sums, want["sums"]) and np.array_equal(got.N, got.count)      # integers: exact however it is cut
        thr = float(np.nanmedian(ld))
        held = p.count_statistics(X, assign=mode, min_logdens=thr)
        want_h, _ = whole_reference(p, X, mode, thr)
        assert held.held_out == int((ld < np.float32(thr)).sum()) > 0 and held.held_out + held.skipped + held.count.sum() == N
        assert C.within(held, want_h, N) <= 1 and np.array_equal(held.count, want_h["count"])
        e = p.count_statistics(X[:, :0])
        assert e.sums.shape == (K, D) and not e.sums.any() and not e.N.any() and e.count.tolist() == [0] * K and e[3:] == (0, 0, 0)
        for kw in (dict(assign="both"), dict(min_logdens=float("nan"))):
            with pytest.raises(ValueError):
                p.count_statistics(X, **kw)
        with pytest.raises(ValueError, match="dimension"):
            p.count_statistics(np.zeros((D + 1, 5), np.float32))
    with pytest.raises(RuntimeError, match="closed"):
        p.count_statistics(X)


def test_niw_predictor_one_shot_and_a_worker_that_cannot(score, host):
    X = counts(50, 6)
    s = types.SimpleNamespace(K=K, prior=types.SimpleNamespace(kind=1, dim=D), post=dict(alpha=np.repeat(alpha_post()["alpha"], 3, axis=0)), alpha=10.0, points_count=np.full(K, 20),
                              wk=types.SimpleNamespace(device=0))
    mdl = types.SimpleNamespace(sampler=s)
    before = len(R.TableWorker.made)
    a = score.count_statistics(mdl, X, capacity=16, worker_factory=CountWorker, assign="soft", min_logdens=-1e30)
    assert len(R.TableWorker.made) == before + 1 and R.TableWorker.made[-1].closed       # the one-shot call closes its worker
    with score.Predictor(mdl, capacity=64, worker_factory=CountWorker) as p:
        b = p.count_statistics(X, assign="soft")
    assert np.allclose(a.sums, b.sums, rtol=1e-13, atol=1e-13) and np.allclose(a.N, b.N, rtol=1e-13) and np.array_equal(a.count, b.count)

    class Cannot(R.TableWorker):                                                     # a worker without countstats_begin
        def set_predictive_mult(self, logp, weights):
            pass
    with open_mult(score, 64, factory=Cannot) as p:
        with pytest.raises(RuntimeError, match="count statistics"):
            p.count_statistics(X)
    made = []

    class NiwWorker(CountWorker):
        def set_predictive_niw(self, *a):
            made.append(self)
    with score.Predictor(R.model(3, K), capacity=16, worker_factory=NiwWorker) as niw:
        for call in (niw.count_statistics, niw.absorb_counts):
            with pytest.raises(ValueError, match="Multinomial"):
                call(np.ones((3, 4), np.float32))
        assert made and not hasattr(made[0], "cs_calls")                             # refused before the worker was asked


def test_absorb_counts_updates_the_model_reloads_once_and_survives_save_and_load(score, tmp_path):
    X = counts(60, 8)
    with open_mult(score, 16) as p:
        wk = p._wk
        assert wk.loads == 1
        p._sampler_set = True                                                        # as after a first sample()
        old_post, old_count, old_w = {k: v.copy() for k, v in p.post.items()}, p.points_count.copy(), p.weights.copy()
        want = p.count_statistics(X, assign="soft")
        got = p.absorb_counts(X, assign="soft")
        assert wk.loads == 2 and p._wk is wk                                         # once, into the same worker
        assert all(np.array_equal(a, b) for a, b in zip(got, want))                  # it absorbed what count_statistics reports
        ref_post, ref_count = score.dirichlet_absorb(old_post, old_count, want)
        assert p.post["alpha"].dtype == np.float64 and p.post["alpha"].tobytes() == ref_post["alpha"].tobytes() and np.array_equal(p.points_count, ref_count)
        assert p.points_count.sum() == pytest.approx(old_count.sum() + 60) and not np.array_equal(p.weights, old_w)
        w = p.points_count + p.alpha
        assert np.array_equal(p.weights, (w / w.sum()).astype(np.float32))
        a64 = ref_post["alpha"]
        assert np.array_equal(wk.logp, np.log(a64 / a64.sum(1, keepdims=True)).astype(np.float32)) and np.array_equal(wk.logw, np.log(p.weights))
        assert not p._sampler_set                                                    # the alias tables of `sample` are stale
        # statistics with no weight change nothing and reload nothing
        none = p.absorb_counts(np.full((D, 5), np.nan, np.float32))
        assert none.skipped == 5 and none.N.sum() == 0 and wk.loads == 2
        assert p.post["alpha"].tobytes() == ref_post["alpha"].tobytes() and np.array_equal(p.points_count, ref_count)
        path = str(tmp_path / "absorbed.npz")
        p.save(path)
        table = wk.logp.copy()
    with score.Predictor.load(path, capacity=16, worker_factory=CountWorker) as q:     # a Float64 alpha round-trips: the same predictive bits
        assert q.post["alpha"].dtype == np.float64 and q.post["alpha"].tobytes() == ref_post["alpha"].tobytes() and np.array_equal(q.points_count, ref_count)
        assert q._wk.loads == 1 and q._wk.logp.tobytes() == table.tobytes()
        again = q.absorb_counts(X, assign="hard")                                    # and goes on absorbing
        assert q._wk.loads == 2 and np.array_equal(again.N, again.count.astype(np.float64))
        assert np.array_equal(q.post["alpha"], ref_post["alpha"] + again.sums)
