"""CPU-side checks of the count explanations (include/dpmm_hip_count_explain.h): the header compiles as C, its functions are bound, exported
and built from csrc/count_explain.hip; the reference (tests/tools/count_explain_ref.py) on cases computed by hand; csrc/count_explain_math.h
with the new general I_x(a, b) of csrc/typicality_math.h compiled into a stand-alone host program and held to the tail contract against
mpmath at 50 digits; `Predictor.explain_counts` over a stand-in worker around tests/fake_worker.py: the refusals, the slab walk with the
short slab's first rows copied and its padding taken off the counters, the tables re-formed after `absorb_counts`."""
import ctypes
import importlib
import os
import re
import subprocess
import types

import mpmath
import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package
from tools import overlap_ref
from tools import count_explain_ref as CR
import test_countstats_cpu as CS
import test_rank_cpu as R

HEADER = os.path.join(ROOT, "include", "dpmm_hip_count_explain.h")
CSRC = os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc")
FUNCS = ["dpmm_count_explain_points", "dpmm_count_explain_points_device", "dpmm_set_count_explain"]
D, K = CS.D, CS.K
FIELDS = ("features", "count", "expected", "residual", "feature_tail", "labels", "total")


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
    assert sorted(n for n, _, _ in binding.ABI_COUNT_EXPLAIN) == FUNCS
    assert "#define DPMM_COUNT_EXPLAIN_MAX_TOP DPMM_SCORE_MAX_TOP" in hdr and binding.COUNT_EXPLAIN_MAX_TOP == binding.SCORE_MAX_TOP == 16
    for name, v in binding.COUNT_EXPLAIN_SIDES.items():
        assert f"#define DPMM_COUNT_EXPLAIN_{name.upper()} {v}" in hdr
    struct = body[body.index("typedef struct {"):body.index("} dpmm_count_explain_out;")]
    fields = re.findall(r"(float|double|int64_t|int32_t|int)\s*(\*?)\s*([A-Za-z_]+);", struct)
    assert [f[2] for f in fields] == [f[0] for f in binding.CountExplainOut._fields_]
    ctype = {("int", ""): ctypes.c_int, ("int64_t", ""): ctypes.c_int64}
    assert [ctype.get((t, p), ctypes.c_void_p) for t, p, _ in fields] == [f[1] for f in binding.CountExplainOut._fields_]
    for name in ("set_count_explain", "count_explain_points_into"):
        assert callable(getattr(binding.Worker, name)), name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "build/count_explain.o" in re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "../../include/dpmm_hip_count_explain.h" in re.search(r"^build/dpmm_api\.o:(.*)$", mk, flags=re.M).group(1).split()
    hip = open(os.path.join(CSRC, "count_explain.hip")).read()
    assert "DPMM_LAUNCH((count_explain_kernel" in hip and "DPMM_LAUNCH(count_explain_finish_kernel" in hip      # the poison hook covers both
    assert "atomicAdd" not in hip and "__syncthreads" not in hip and "__shared__" not in hip                  # one writer per word; the waves share nothing
    assert "cs_wave_total" in hip and '#include "count_explain_math.h"' in hip
    jl = open(os.path.join(ROOT, "julia", "gpu_count_explain.jl")).read()
    assert set(re.findall(r":(dpmm_[a-z0-9_]+)", jl)) == set(FUNCS)
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for n in FUNCS:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                               # additive: the version stays
    assert host.CountExplanation is score.CountExplanation and host.explain_counts is score.explain_counts and callable(host.Predictor.explain_counts)
    assert score.CountExplanation._fields == FIELDS + ("skipped", "incomplete")


# ---------------------------------------------------------------------------------------------- the reference on cases computed by hand
def test_reference_on_hand_computed_cases():
    # t = 4, theta = 1/4: x = 0 under, (3/4)^4; x = 1 = t theta: equal, g = 0, tail 1; x = 2 over, P(X >= 2) = 67/256; x = 4 over, (1/4)^4
    x, t, th = np.array([0.0, 1.0, 2.0, 4.0]), 4.0, 0.25
    s = CR.side_of(x, t, th)
    assert s.tolist() == [-1, 0, 1, 1]
    g, A = CR.deviance(x, t, th)
    want = [-8 * np.log(0.75), 0.0, 2 * (2 * np.log(2.0) + 2 * np.log(2.0 / 3.0)), 8 * np.log(4.0)]
    assert np.allclose(g, want, rtol=1e-15, atol=1e-16) and (A > 0).all()
    for xi, si, w in zip(x, s, (81 / 256, 1.0, 67 / 256, 1 / 256)):
        assert abs(float(CR.tail_mp(xi, t, th, si)) - w) < 1e-16
    assert np.allclose(CR.tail_fast(x, t, th, s), [81 / 256, 1.0, 67 / 256, 1 / 256], rtol=1e-14)
    # the ranking: the deviance, not the z-score.  A rare feature seen once (z = 100, tail 1e-4) ranks BELOW a common one at four times its expectation
    th2 = np.array([1e-6, 0.1, 1 - 0.1 - 1e-6])
    x2 = np.array([1.0, 40.0, 59.0])
    g2, _ = CR.deviance(x2, 100.0, th2)
    z = (x2 - 100 * th2) / np.sqrt(100 * th2)
    assert z[0] > z[1] and g2[1] > g2[0]
    r = (CR.side_of(x2, 100.0, th2) * np.sqrt(g2)).astype(np.float32)
    assert CR.topm(r, r > 0, 2).tolist() == [1, 0] and CR.topm(r, r < 0, 2).tolist() == [2, -1]
    assert CR.topm(np.array([1.0, -1.0, 0.5, 1.0], np.float32), np.ones(4, bool), 3).tolist() == [0, 1, 3]      # ties to the lower index
    # the whole definition on a dense matrix, and the checker on its own output
    X = np.array([[0, 1, 2, 4], [4, 3, 2, 0], [0, 0, 0, 0]], np.float64)
    X[:, 3] = [0, 0, 0]                                                  # an empty point: incomplete
    theta = np.array([[0.25, 0.5, 0.25]])
    lab = np.ones(4, np.int64)
    F, C, E, Rr, T = CR.explain(X, lab, theta, 2, "both")
    assert F[0].tolist() == [1, 0] and F[3].tolist() == [-1, -1] and np.isnan(T[3]).all()
    got = types.SimpleNamespace(features=F, count=C, expected=E, residual=Rr, feature_tail=T, labels=lab, total=X.sum(0), skipped=0, incomplete=1)
    assert CR.check(got, X, theta, 2, "both")[0] <= 1.0
    bad = types.SimpleNamespace(**vars(got))
    bad.features = F.copy()
    bad.features[0] = [2, 0]                                             # feature 2 (|r| smaller) instead of feature 1
    with pytest.raises(AssertionError):
        CR.check(bad, X, theta, 2, "both")
    bad = types.SimpleNamespace(**vars(got))
    bad.feature_tail = T * np.float32(1 + 2.0 ** -18)
    with pytest.raises(AssertionError, match="tail"):
        CR.check(bad, X, theta, 2, "both")


# ---------------------------------------------------------------------------------------------- the device arithmetic as a host program
def test_host_build_of_the_tail_meets_the_contract_on_a_grid(tmp_path):
    exe = str(tmp_path / "count_explain_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "tools", "count_explain_host.cpp"), "-o", exe])
    grid = []
    for t in (1.0, 2.0, 7.0, 100.0, 3000.0, 1e6):
        for th in (1e-9, 1e-6, 1e-3, 0.03, 0.25, 0.5, 0.9, 1 - 1e-6):
            e = t * th
            xs = {0.0, 1.0, t, np.floor(e), np.ceil(e), np.ceil(e + 3 * np.sqrt(e) + 1), max(0.0, np.floor(e - 3 * np.sqrt(e))), np.ceil(4 * e), np.floor(t / 2)}
            grid += [(x, t, th) for x in sorted(xs) if 0 <= x <= t]
    grid += [(1.0, 1e6, 1e-9), (0.0, 1e6, 1e-9), (1e6, 1e6, 0.999), (3.5, 10.25, 0.2)]      # ... and a value that is no integer
    out = subprocess.run([exe], input="".join(f"{float(x)!r} {float(t)!r} {float(th)!r}\n" for x, t, th in grid), capture_output=True, text=True, check=True).stdout.split("\n")
    worst, worst_g, most_trips = 0.0, 0.0, 0
    for (x, t, th), line in zip(grid, out):
        side, r, g, tail, trips, ib = line.split()
        side, r, g, tail, trips, ib = int(side), float(r), float(g), float(tail), int(trips), float(ib)
        assert side == int(CR.side_of(x, t, th)), (x, t, th)
        gs, A = CR.deviance(x, t, th)
        assert abs(g - gs) <= 16 * CR.U * A, (x, t, th, g, gs)
        worst_g = max(worst_g, abs(g - float(gs)) / (16 * CR.U * float(A)))
        if side != 0:
            assert np.sqrt(max(gs - 16 * CR.U * A, 0)) * (1 - CR.EPS32) <= r <= np.sqrt(gs + 16 * CR.U * A) * (1 + CR.EPS32), (x, t, th)
        for got, ex in ((tail, CR.tail_mp(x, t, th, side)),) + (((ib, CR.tail_mp(x, t, th, 1)),) if ib >= 0 and side > 0 else ()):
            if ex >= CR.TAIL_FLOOR:
                err = float(abs(mpmath.mpf(got) - ex) / ex)
                assert err <= CR.TAIL_REL / 2, (x, t, th, got, ex)             # (half the contract: the Float32 rounding is still to come)
                worst = max(worst, err)
            else:
                assert 0 <= got <= CR.TAIL_FLOOR * (1 + CR.TAIL_REL), (x, t, th, got, ex)
        most_trips = max(most_trips, trips)
    print(len(grid), "cases; worst relative tail error", worst, "; worst |g - g*| in units of its bound", worst_g, "; most trips", most_trips)
    assert most_trips < 20000


# ---------------------------------------------------------------------------------------------- Predictor.explain_counts over a stand-in
class ExplainWorker(CS.CountWorker):
    """The table-keeping Multinomial stand-in (tests/fake_worker.py underneath) with the two calls `Predictor.explain_counts` makes, answered
    by tests/tools/count_explain_ref.py from the tables it was handed."""

    def set_predictive_mult(self, logp, weights):
        super().set_predictive_mult(logp, weights)
        self.ce_tables = None                                                    # a later set_predictive_* invalidates the tables

    def set_count_explain(self, log_theta, log1m_theta, order):
        lth, l1m, order = np.asarray(log_theta), np.asarray(log1m_theta), np.asarray(order)
        assert lth.dtype == l1m.dtype == np.float64 and order.dtype == np.int32 and lth.shape == l1m.shape == order.shape == (self.K, self.D)
        for k in range(self.K):
            assert sorted(order[k].tolist()) == list(range(self.D)) and (np.diff(l1m[k, order[k]]) >= 0).all()
        self.ce_tables = (lth, l1m, order)
        self.ce_sets = getattr(self, "ce_sets", []) + [lth.copy()]

    def count_explain_points_into(self, views, top, side="both"):
        assert self.ce_tables is not None, "DPMM_ESTATE: needs dpmm_set_count_explain"
        self.ce_calls = getattr(self, "ce_calls", []) + [(int(top), side)]
        P, lab, part = overlap_ref.probs(self.table())
        X = self.X.T.astype(np.float64)
        F, C, E, Rr, T = CR.explain(X, lab, np.exp(self.ce_tables[0]), top, side)
        for a in (C, E, Rr, T):
            a[~part] = np.nan
        F[~part] = -1
        with np.errstate(all="ignore"):
            tot = np.where(part, X.sum(0), np.nan)
            ok = np.isfinite(X).all(0) & (X >= 0).all(0) & (X.sum(0) > 0)
        for name, a in (("features", F), ("count", C), ("expected", E), ("residual", Rr), ("feature_tail", T), ("labels", lab), ("total", tot)):
            assert views[name].shape == a.shape, name
            views[name][:] = a
        return int((~part).sum()), int((part & ~ok).sum())


N = 29


def open_mult(score, cap, **kw):
    return CS.open_mult(score, cap, factory=ExplainWorker, **kw)


def whole(p, X, top, side):
    """What one worker holding all the points answers."""
    w = ExplainWorker(1, X.shape[0], X.shape[1])
    w.logp, w.logw, w.K = p._wk.logp, p._wk.logw, p._wk.K
    w.ce_tables = p.count_explain_tables()
    w.upload_points(np.ascontiguousarray(X.T))
    n = X.shape[1]
    views = dict(features=np.empty((n, top), np.int32), labels=np.empty(n, np.int64), total=np.empty(n), **{f: np.empty((n, top), np.float32) for f in FIELDS[1:5]})
    return views, w.count_explain_points_into(views, top, side)


@pytest.mark.parametrize("cap", [1, 7, N, N + 5])
def test_predictor_explain_counts_walks_the_slabs(score, cap):
    X = CS.counts(N, 5)
    X[1, 11] = np.nan                                                            # a NaN row of the table: skipped
    X[:, 3] = 0.0                                                                # an empty point: incomplete, as the padding of a short slab is
    with open_mult(score, cap) as p:
        wk = p._wk
        for top, side in ((2, "both"), (D, "over"), (3, "under")):
            want, (sk, inc) = whole(p, X, top, side)
            got = p.explain_counts(X, top, side=side)
            assert isinstance(got, score.CountExplanation) and isinstance(got.skipped, int) and isinstance(got.incomplete, int)
            assert got.features.shape == (N, top) and got.features.dtype == np.int32 and got.total.dtype == np.float64 and got.labels.dtype == np.int64
            for f in FIELDS:                                                     # the short slab's first rows
                assert np.asarray(getattr(got, f)).tobytes() == want[f].tobytes(), f
            assert (got.skipped, got.incomplete) == (sk, inc) == (1, 1)          # the padding is not counted
            assert (got.features[[3, 11]] == -1).all() and np.isnan(got.total[11]) and got.total[3] == 0
        assert all(u == cap for u in wk.uploads)                                 # never a short upload
        assert len(wk.ce_sets) == 1                                              # the tables are formed once
        lth, l1m, order = p.count_explain_tables()
        th = CR.theta_of(p.post["alpha"])
        assert lth.tobytes() == np.log(th).tobytes() and l1m.tobytes() == np.log1p(-th).tobytes() and th.tobytes() == p.sampler_tables()[1].tobytes()
        assert order.dtype == np.int32 and all((np.diff(l1m[k, order[k]]) >= 0).all() for k in range(K))
        e = p.explain_counts(X[:, :0], 2)
        assert e.features.shape == (0, 2) and e.total.shape == (0,) and (e.skipped, e.incomplete) == (0, 0)


def test_refusals(score):
    X = CS.counts(10, 6)
    with open_mult(score, 8) as p:
        for top in (0, -1, D + 1, 17, 1.5):
            with pytest.raises(ValueError, match=f"1..{D}"):
                p.explain_counts(X, top)
        with pytest.raises(ValueError, match="side"):
            p.explain_counts(X, 2, side="two")
        with pytest.raises(ValueError, match="dimension"):
            p.explain_counts(np.zeros((D + 1, 5), np.float32), 2)
        assert not hasattr(p._wk, "ce_calls")                                    # refused before the worker was asked
        p.projection = object()                                                  # a model with a projection
        with pytest.raises(ValueError, match="projection"):
            p.explain_counts(X, 2)
        p.projection = None
    with pytest.raises(RuntimeError, match="closed"):
        p.explain_counts(X, 2)
    wide = score.Predictor.__new__(score.Predictor)
    wide._setup(1, 40, 10.0, np.full(2, 20.0), dict(alpha=np.ones((2, 40), np.float32)), 8, 0, ExplainWorker)
    with wide:
        with pytest.raises(ValueError, match="1..16"):                           # min(D, 16)
            wide.explain_counts(np.ones((40, 3), np.float32), 17)
        assert wide.explain_counts(np.ones((40, 3), np.float32), 16).features.shape == (3, 16)
    made = []

    class NiwWorker(ExplainWorker):
        def set_predictive_niw(self, *a):
            made.append(self)
    with score.Predictor(R.model(3, K), capacity=16, worker_factory=NiwWorker) as niw:
        with pytest.raises(ValueError, match="Multinomial"):
            niw.explain_counts(np.ones((3, 4), np.float32), 1)
        assert made and not hasattr(made[0], "ce_calls")

    class Cannot(CS.CountWorker):                                                # a worker without the call
        pass
    with CS.open_mult(score, 8, factory=Cannot) as p:
        with pytest.raises(RuntimeError, match="dpmm_count_explain_points"):
            p.explain_counts(X, 2)


def test_one_shot_and_the_tables_are_reformed_after_absorb_counts(score, host):
    X = CS.counts(60, 8)
    Y = CS.counts(20, 9)
    with open_mult(score, 16) as p:
        wk = p._wk
        before = p.explain_counts(Y, 3)
        assert p._count_explain_set and len(wk.ce_sets) == 1
        p.absorb_counts(X, assign="soft")
        assert not p._count_explain_set and wk.ce_tables is None                 # the worker's tables went with the reload
        after = p.explain_counts(Y, 3)
        assert len(wk.ce_sets) == 2 and wk.ce_sets[1].tobytes() == np.log(CR.theta_of(p.post["alpha"])).tobytes()
        assert wk.ce_sets[1].tobytes() != wk.ce_sets[0].tobytes() and after.expected.tobytes() != before.expected.tobytes()
        p.explain_counts(Y, 3)
        assert len(wk.ce_sets) == 2                                              # ... and only then
    s = types.SimpleNamespace(K=K, prior=types.SimpleNamespace(kind=1, dim=D), post=dict(alpha=np.repeat(CS.alpha_post()["alpha"], 3, axis=0)), alpha=10.0,
                              points_count=np.full(K, 20), wk=types.SimpleNamespace(device=0))
    n_made = len(R.TableWorker.made)
    one = host.explain_counts(types.SimpleNamespace(sampler=s), Y, 3, side="over", capacity=16, worker_factory=ExplainWorker)
    assert len(R.TableWorker.made) == n_made + 1 and R.TableWorker.made[-1].closed      # the one-shot call closes its worker
    with open_mult(score, 64) as q:
        two = q.explain_counts(Y, 3, side="over")
    assert np.array_equal(one.features, two.features) and one.residual.tobytes() == two.residual.tobytes()
