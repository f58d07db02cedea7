"""CPU-side checks of the batch statistics (include/dpmm_hip_batchstats.h) and of the conjugate update (host/absorb.py): the header
compiles as C, its functions are bound, exported and built from csrc/batchstats.hip; `niw_absorb` against the centred formulation of
tests/tools/batchstats_ref.py, its conjugacy, untouched clusters and refusals; `Predictor.statistics` / `absorb` over a stand-in worker
that keeps a numpy table: the slab walk, the Multinomial refusal, one reload of the predictives per absorb, the save / load round trip."""
import ctypes
import importlib
import os
import re
import subprocess
import types

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package
from tools import batchstats_ref as B
from tools import overlap_ref, rank_ref
import test_rank_cpu as R

HEADER = os.path.join(ROOT, "include", "dpmm_hip_batchstats.h")
FUNCS = ["dpmm_batchstats_accumulate", "dpmm_batchstats_begin", "dpmm_batchstats_read"]


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
def test_header_compiles_as_c_and_is_bound_exported_and_built(pkg, host):
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER])
    hdr = open(HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", body))) == FUNCS
    binding = importlib.import_module(pkg.__name__ + ".binding")
    assert sorted(n for n, _, _ in binding.ABI_BATCHSTATS) == FUNCS
    others = (binding.ABI + binding.ABI_TENSOR + binding.ABI_SCORE + binding.ABI_RANK + binding.ABI_OVERLAP + binding.ABI_TRACE + binding.ABI_MISSING
              + binding.ABI_IMPUTE + binding.ABI_CSC + binding.ABI_SAMPLE + binding.ABI_PROJECT)
    assert not set(FUNCS) & set(n for n, _, _ in others)
    for name in ("batchstats_begin", "batchstats_accumulate", "batchstats_read", "batchstats_read_raw"):
        assert callable(getattr(binding.Worker, name)), name
    assert int(re.search(r"#define DPMM_BATCHSTATS_PARTIAL_BLOCKS (\d+)", hdr).group(1)) == binding.BATCHSTATS_PARTIAL_BLOCKS
    assert int(re.search(r"#define DPMM_BATCHSTATS_HARD (\d+)", hdr).group(1)) == binding.BATCHSTATS_HARD
    assert int(re.search(r"#define DPMM_BATCHSTATS_SOFT (\d+)", hdr).group(1)) == binding.BATCHSTATS_SOFT
    struct = body[body.index("typedef struct {"):body.index("} dpmm_batchstats_out;")]
    assert re.findall(r"\*\s*([A-Za-z_]+);", struct) == [f[0] for f in binding.BatchStatsOut._fields_]
    assert re.findall(r"(double|int64_t)\s*\*", struct) == ["double"] * 3 + ["int64_t"] * 4
    csrc = os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "build/batchstats.o" in re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "../../include/dpmm_hip_batchstats.h" in re.search(r"^build/dpmm_api\.o:(.*)$", mk, flags=re.M).group(1).split()
    kern = open(os.path.join(csrc, "dpmm_kernels.h")).read()
    assert int(re.search(r"BATCHSTATS_PARTIAL_BLOCKS = (\d+)", kern).group(1)) == binding.BATCHSTATS_PARTIAL_BLOCKS
    hip = open(os.path.join(csrc, "batchstats.hip")).read()
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in hip and "atomicAdd(&A.acc" not in hip and '#include "score_device.h"' in hip
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for n in FUNCS:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                               # additive: the version stays
    assert callable(host.statistics) and callable(host.niw_absorb) and callable(host.Predictor.statistics) and callable(host.Predictor.absorb)
    assert host.BatchStatistics._fields == ("N", "sums", "S", "count", "skipped", "incomplete", "held_out")


# ---------------------------------------------------------------------------------------------- the reference itself
def test_batchstats_ref_on_points_written_by_hand():
    nan, inf = np.nan, np.inf
    #              0    1    2    3    4     5
    X = np.array([[1.0, 2.0, 3.0, nan, 5.0, -1.0],
                  [0.5, 0.0, inf, 1.0, 1.0, 2.0]], np.float32)
    P = np.array([[1, 0], [.25, .75], [.5, .5], [1, 0], [nan, nan], [0, 1]], np.float32)
    lab = np.array([1, 2, 1, 1, 1, 2])
    ld = np.array([-1.0, -9.0, -1.0, -1.0, nan, -2.0], np.float32)
    # point 2: an Inf feature, 3: a NaN feature under a finite row (marginalised), 4: skipped, 1: below the floor -8
    sk, held, inc, part = B.classes(X, P, ld, -8.0)
    assert sk.tolist() == [0, 0, 0, 0, 1, 0] and held.tolist() == [0, 1, 0, 0, 0, 0] and inc.tolist() == [0, 0, 1, 1, 0, 0]
    assert part.tolist() == [1, 0, 0, 0, 0, 1]
    r = B.stats(X, lab, P, "hard", ld, -8.0)
    assert (r["skipped"], r["held_out"], r["incomplete"], r["count"].tolist()) == (1, 1, 2, [1, 1])
    assert r["N"].tolist() == [1, 1] and r["sums"].tolist() == [[1, .5], [-1, 2]] and r["S"][1].tolist() == [[1, -2], [-2, 4]]
    assert r["T"][1].tolist() == [[1, 2], [2, 4]] and r["T1"][1].tolist() == [1, 2]
    s = B.stats(X, lab, P, "soft")                                  # no floor: point 1 takes part with (1/4, 3/4)
    assert s["held_out"] == 0 and s["count"].tolist() == [1, 2] and s["N"].tolist() == [1.25, 1.75]
    assert s["sums"][0].tolist() == [1 + .25 * 2, .5] and s["S"][0].tolist() == [[2, .5], [.5, .25]]
    assert B.within(s, s, 6) == 0 and B.within(dict(s, N=s["N"] * (1 + 2.0 ** -40)), s, 6) > 1
    both = B.add([B.stats(X[:, :3], lab[:3], P[:3], "soft"), B.stats(X[:, 3:], lab[3:], P[3:], "soft")])
    assert B.within(both, s, 6) <= 1 and both["count"].tolist() == [1, 2] and both["incomplete"] == 2
    assert B.gamma(1) == 2.0 ** -53 / (1 - 2.0 ** -53)


# ---------------------------------------------------------------------------------------------- niw_absorb
def absorb_case(D, K, seed, soft=False):
    """Random well-conditioned posteriors and weighted Float32 points per cluster: (post, points_count, per-cluster (w, x), stats dict)."""
    rng = np.random.default_rng(seed)
    U = np.triu(rng.standard_normal((K, D, D)) * 0.1) + 2 * np.eye(D)
    nu = D + 3 + 50 * rng.random(K)
    post = dict(kappa=1 + 50 * rng.random(K), nu=nu, m=rng.standard_normal((K, D)) * 3, U=U,
                logdet_psi=2 * np.log(np.einsum("kii->ki", U)).sum(1) - D * np.log(nu))
    count = rng.integers(50, 500, K).astype(np.float64)
    data = []
    for k in range(K):
        n = int(rng.integers(40, 400))
        x = (post["m"][k] + rng.standard_normal(D) + rng.standard_normal((n, D))).astype(np.float32).astype(np.float64)
        w = rng.random(n).astype(np.float32).astype(np.float64) if soft else np.ones(n)
        data.append((w, x))
    stats = dict(N=np.array([w.sum() for w, _ in data]), sums=np.stack([(w[:, None] * x).sum(0) for w, x in data]),
                 S=np.stack([(w[:, None] * x).T @ x for w, x in data]))
    return post, count, data, stats


def formulation_gap(post, data, stats):
    """The largest relative difference (max |a - b| / max |b| per cluster) between the centred and the uncentred Float64 formulation."""
    gap = 0.0
    cen = []
    for k, (w, x) in enumerate(data):
        Psi = post["U"][k] @ post["U"][k].T
        a = B.update_centred(post["kappa"][k], post["nu"][k], post["m"][k], Psi, w, x)
        b = B.update_uncentred(post["kappa"][k], post["nu"][k], post["m"][k], Psi, stats["N"][k], stats["sums"][k], stats["S"][k])
        gap = max(gap, B.rel(b[3], a[3]), B.rel(b[2], a[2]))
        cen.append(a)
    return gap, cen


@pytest.mark.parametrize("D", [2, 17, 64])
@pytest.mark.parametrize("soft", [False, True])
def test_niw_absorb_equals_the_centred_update(host, D, soft):
    """Tolerance: 8 x the largest relative difference between the reference's centred and uncentred Float64 formulations on the same
    inputs -- the two differ only in rounding, and so does the library's arithmetic from either.  Measured on these inputs (hard / soft):
    D = 2: gap 2.79e-13 / 4.51e-14, D = 17: 2.77e-13 / 3.60e-14, D = 64: 2.72e-13 / 1.16e-13 -- tolerances 2.9e-13 .. 2.2e-12 (the
    uncentred form cancels kappa m m' + S against kappa' m' m''); niw_absorb lies at 0.12 .. 0.15 of its tolerance."""
    K = 5
    post, count, data, stats = absorb_case(D, K, 100 + D, soft)
    gap, cen = formulation_gap(post, data, stats)
    tol = 8 * gap
    new, cnt = host.niw_absorb(post, count, types.SimpleNamespace(**stats))
    worst = 0.0
    for k, (k1, nu1, m1, Psi1) in enumerate(cen):
        U1 = new["U"][k]
        assert np.array_equal(U1, np.triu(U1)) and (np.diag(U1) > 0).all()                         # the convention of niw_hyperparams.posterior
        worst = max(worst, B.rel(U1 @ U1.T, Psi1), B.rel(new["m"][k], m1))
        assert abs(new["kappa"][k] - k1) <= tol * k1 and abs(new["nu"][k] - nu1) <= tol * nu1
        sign, ld = np.linalg.slogdet(Psi1 / nu1)
        assert sign > 0 and abs(new["logdet_psi"][k] - ld) <= tol * D * np.linalg.cond(Psi1)
    print(f"D = {D} soft = {soft}: formulation gap {gap:.3g}, tolerance {tol:.3g}, niw_absorb at {worst / tol:.3g} of it")
    assert 0 < gap < 1e-11 and worst <= tol      # (the ceiling: 2^-53 times a cancellation of 1e5 between S, kappa m m' and kappa' m' m'' -- a tolerance beyond it would check nothing)
    assert np.allclose(cnt, count + stats["N"], rtol=0, atol=0)
    for k in ("kappa", "nu", "m", "U", "logdet_psi"):
        assert new[k].dtype == np.float64 and new[k] is not post[k]
    # the native route keeps Float64 kappa and nu: a fractional N far below Float32 resolution is not lost
    if soft:
        assert np.all(new["kappa"] - post["kappa"] == (post["kappa"] + stats["N"]) - post["kappa"])


@pytest.mark.parametrize("D", [2, 17, 64])
def test_conjugacy_and_untouched_clusters(host, D):
    K = 4
    post, count, data, sA = absorb_case(D, K, 200 + D, soft=True)
    _, _, dataB, sB = absorb_case(D, K, 300 + D, soft=True)
    both = [(np.concatenate([wa, wb]), np.concatenate([xa, xb])) for (wa, xa), (wb, xb) in zip(data, dataB)]
    sAB = {f: sA[f] + sB[f] for f in sA}
    tol = 8 * max(formulation_gap(post, both, sAB)[0], formulation_gap(post, data, sA)[0])
    one, c1 = host.niw_absorb(post, count, sAB)
    mid, cm = host.niw_absorb(post, count, sA)
    two, c2 = host.niw_absorb(mid, cm, sB)
    for k in range(K):
        assert B.rel(two["U"][k] @ two["U"][k].T, one["U"][k] @ one["U"][k].T) <= tol and B.rel(two["m"][k], one["m"][k]) <= tol
    assert np.all(np.abs(two["kappa"] - one["kappa"]) <= tol * one["kappa"]) and np.all(np.abs(two["nu"] - one["nu"]) <= tol * one["nu"])
    assert np.all(np.abs(c2 - c1) <= tol * c1)
    # clusters without weight keep their bits, whatever sums and S say
    z = {f: v.copy() for f, v in sA.items()}
    z["N"][[1, 3]] = 0.0
    got, c = host.niw_absorb(post, count, z)
    for f in ("kappa", "nu", "m", "U", "logdet_psi"):
        assert got[f][[1, 3]].tobytes() == np.asarray(post[f], np.float64)[[1, 3]].tobytes(), f
        assert not np.array_equal(got[f][0], post[f][0]), f
    assert c[[1, 3]].tolist() == count[[1, 3]].tolist() and c[0] == count[0] + z["N"][0]
    same, c0 = host.niw_absorb(post, count, {f: np.zeros_like(v) for f, v in sA.items()})
    assert all(same[f].tobytes() == np.asarray(post[f], np.float64).tobytes() for f in same) and c0.tolist() == count.tolist()


def test_niw_absorb_refusals(host):
    post, count, _, s = absorb_case(3, 2, 7)
    for bad in (dict(s, N=s["N"][:1]), dict(s, sums=s["sums"][:, :2]), dict(s, S=s["S"][:, :2]), dict(s, N=-s["N"]), dict(s, N=s["N"] * np.nan),
                dict(s, sums=s["sums"] * np.inf), dict(s, S=s["S"] * np.nan)):
        with pytest.raises(ValueError):
            host.niw_absorb(post, count, bad)
    with pytest.raises(ValueError, match="points_count"):
        host.niw_absorb(post, count[:1], s)
    with pytest.raises(ValueError, match="NIW"):
        host.niw_absorb(dict(alpha=np.ones((2, 3))), count, s)
    with pytest.raises(ValueError, match="positive definite"):
        host.niw_absorb(post, count, dict(s, S=-1e6 * s["S"]))
    nold = {k: v for k, v in post.items() if k != "logdet_psi"}                 # a model file written without logdet_psi: computed from U and nu
    assert np.allclose(host.niw_absorb(nold, count, dict(s, N=s["N"] * 0))[0]["logdet_psi"], post["logdet_psi"], rtol=1e-14)


# ---------------------------------------------------------------------------------------------- Predictor.statistics / absorb over a stand-in
class BatchWorker(R.TableWorker):
    """tests/test_rank_cpu.py's table-keeping stand-in with the calls `Predictor.statistics` makes, piece by piece through batchstats_ref."""

    def set_predictive_niw(self, m, R_, logdet, df, weights):
        super().set_predictive_niw(m, R_, logdet, df, weights)
        self.loads = getattr(self, "loads", 0) + 1
        self.bs_pieces = None                                                    # another parameter set: an accumulation does not survive it

    def scored(self, n_valid):
        tab = self.table()[:, :n_valid]
        P, lab, part = overlap_ref.probs(tab)
        P[~part] = np.nan                                                        # what `predict` writes for them
        _, M, _ = rank_ref.labels_and_scores(tab)
        with np.errstate(all="ignore"):
            ld = (M + np.log(np.exp(tab - M[None, :]).sum(0))).astype(np.float32)
        return self.X[:n_valid].T, lab, P, ld

    def batchstats_begin(self, mode, min_logdens=None):
        self.bs_mode, self.bs_floor, self.bs_pieces, self.bs_calls = ("hard", "soft")[mode], min_logdens, [], []

    def batchstats_accumulate(self, n_valid):
        assert 0 <= n_valid <= self.n and self.bs_pieces is not None
        self.bs_calls.append(int(n_valid))
        X, lab, P, ld = self.scored(n_valid)
        self.bs_pieces.append(B.stats(X, lab, P, self.bs_mode, ld, self.bs_floor))

    def batchstats_read(self):
        r = B.add(self.bs_pieces) if self.bs_pieces else B.stats(np.zeros((self.D, 0), np.float32), np.zeros(0, np.int64), np.zeros((0, self.K), np.float32), "hard")
        return dict(r, **{f: np.array([r[f]], np.int64) for f in ("skipped", "incomplete", "held_out")})


N = 29


def whole_reference(p, X, mode, floor=None):
    whole = BatchWorker(0, X.shape[0], X.shape[1])
    whole.centres, whole.logw, whole.K = p._wk.centres, p._wk.logw, p._wk.K
    whole.upload_points(np.ascontiguousarray(X.T))
    Xs, lab, P, ld = whole.scored(X.shape[1])
    return B.stats(Xs, lab, P, mode, ld, floor), ld


@pytest.mark.parametrize("cap", [1, 7, N, N + 5])
@pytest.mark.parametrize("mode", ["hard", "soft"])
def test_predictor_statistics_walks_the_slabs(score, cap, mode):
    D, K = 3, 4
    X = np.random.default_rng(5).standard_normal((D, N)).astype(np.float32)
    X[1, 11] = np.nan                                                            # a NaN row of the table: skipped
    with score.Predictor(R.model(D, K), capacity=cap, worker_factory=BatchWorker) as p:
        wk = p._wk
        want, ld = whole_reference(p, X, mode)
        got = p.statistics(X, assign=mode)
        assert isinstance(got, score.BatchStatistics) and all(isinstance(v, int) for v in got[4:]) and all(isinstance(a, np.ndarray) for a in got[:4])
        assert got.S.shape == (K, D, D) and got.sums.shape == (K, D) and got.N.dtype == np.float64 and got.count.dtype == np.int64
        assert wk.uploads == [cap] * -(-N // cap)                                 # never a short upload ...
        assert wk.bs_calls == [min(cap, N - lo) for lo in range(0, N, cap)]      # ... the padding is cut by n_valid
        assert B.within(got, want, N) <= 1 and np.array_equal(got.count, want["count"])
        assert (got.skipped, got.incomplete, got.held_out) == (1, 0, 0) and got.count.sum() == N - 1
        thr = float(np.nanmedian(ld))
        held = p.statistics(X, assign=mode, min_logdens=thr)
        want_h, _ = whole_reference(p, X, mode, thr)
        assert held.held_out == int((ld < np.float32(thr)).sum()) > 0 and held.held_out + held.skipped + held.count.sum() == N
        assert B.within(held, want_h, N) <= 1 and np.array_equal(held.count, want_h["count"])
        e = p.statistics(X[:, :0])
        assert e.S.shape == (K, D, D) and not e.S.any() and not e.N.any() and e.count.tolist() == [0] * K and e[4:] == (0, 0, 0)
        for kw in (dict(assign="both"), dict(min_logdens=float("nan"))):
            with pytest.raises(ValueError):
                p.statistics(X, **kw)
        with pytest.raises(ValueError, match="dimension"):
            p.statistics(np.zeros((D + 1, 5), np.float32))
    with pytest.raises(RuntimeError, match="closed"):
        p.statistics(X)


def test_multinomial_predictor_one_shot_and_a_worker_that_cannot(score, host):
    D, K = 3, 4
    X = np.random.default_rng(6).standard_normal((D, 50)).astype(np.float32)
    mdl = R.model(D, K)
    before = len(R.TableWorker.made)
    a = score.statistics(mdl, X, capacity=16, worker_factory=BatchWorker, assign="soft")
    assert len(R.TableWorker.made) == before + 1 and R.TableWorker.made[-1].closed
    with score.Predictor(mdl, capacity=64, worker_factory=BatchWorker) as p:
        b = p.statistics(X, assign="soft")
    assert np.allclose(a.S, b.S, rtol=1e-13, atol=1e-13) and np.allclose(a.N, b.N, rtol=1e-13) and np.array_equal(a.count, b.count)      # the same sums cut otherwise
    assert host.statistics is score.statistics and host.BatchStatistics is score.BatchStatistics and host.niw_absorb is score.niw_absorb
    with score.Predictor(mdl, capacity=64, worker_factory=R.TableWorker) as p:       # a worker without batchstats_begin
        with pytest.raises(RuntimeError, match="batch statistics"):
            p.statistics(X)
    mult = score.Predictor.__new__(score.Predictor)
    made = []

    class MultWorker(BatchWorker):
        def set_predictive_mult(self, logp, weights):
            made.append(self)
    mult._setup(1, D, 10.0, np.full(K, 5.0), dict(alpha=np.ones((K, D), np.float32)), 16, 0, MultWorker)
    for call in (mult.statistics, mult.absorb):
        with pytest.raises(ValueError, match="NIW"):
            call(np.ones((D, 4), np.float32))
    assert made and not hasattr(made[0], "bs_calls")                                 # refused before the worker was asked
    mult.close()


def test_absorb_updates_the_model_reloads_once_and_survives_save_and_load(score, tmp_path):
    D, K = 3, 4
    rng = np.random.default_rng(8)
    mdl = R.model(D, K)
    U = mdl.sampler.post["U"]
    mdl.sampler.post["logdet_psi"] = 2 * np.log(np.einsum("kii->ki", U)).sum(1) - D * np.log(mdl.sampler.post["nu"])
    X = (mdl.sampler.post["m"][::3][rng.integers(0, K, 60)] + 0.3 * rng.standard_normal((60, D))).T.astype(np.float32)
    with score.Predictor(mdl, capacity=16, worker_factory=BatchWorker) as p:
        wk = p._wk
        assert wk.loads == 1
        old_post, old_count, old_w = {k: v.copy() for k, v in p.post.items()}, p.points_count.copy(), p.weights.copy()
        want = p.statistics(X, assign="soft")
        got = p.absorb(X, assign="soft")
        assert wk.loads == 2 and p._wk is wk                                         # once, into the same worker
        assert all(np.array_equal(a, b) for a, b in zip(got, want))                  # it absorbed what statistics reports
        ref_post, ref_count = score.niw_absorb(old_post, old_count, want)
        assert all(p.post[k].tobytes() == ref_post[k].tobytes() for k in ref_post) and np.array_equal(p.points_count, ref_count)
        assert p.points_count.sum() == pytest.approx(old_count.sum() + 60) and not np.array_equal(p.weights, old_w)
        w = p.points_count + p.alpha
        assert np.array_equal(p.weights, (w / w.sum()).astype(np.float32))
        assert np.array_equal(wk.centres, p.post["m"].astype(np.float32)) and np.array_equal(wk.logw, np.log(p.weights))      # the worker holds the new model
        assert not p._sampler_set
        # statistics with no weight change nothing and reload nothing
        snap = {k: v.copy() for k, v in p.post.items()}
        none = p.absorb(np.full((D, 5), np.nan, np.float32))
        assert none.skipped == 5 and none.N.sum() == 0 and wk.loads == 2
        assert all(p.post[k].tobytes() == snap[k].tobytes() for k in snap) and np.array_equal(p.points_count, ref_count)
        path = str(tmp_path / "absorbed.npz")
        p.save(path)
    with score.Predictor.load(path, capacity=16, worker_factory=BatchWorker) as q:
        assert all(q.post[k].tobytes() == ref_post[k].tobytes() for k in ref_post) and np.array_equal(q.points_count, ref_count)
        assert q._wk.loads == 1 and np.array_equal(q._wk.centres, ref_post["m"].astype(np.float32))
        again = q.absorb(X, assign="hard")                                           # and goes on absorbing
        assert q._wk.loads == 2 and np.array_equal(again.N, again.count.astype(np.float64))
