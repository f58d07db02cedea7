"""CPU-side checks of the next-count recommendations (include/dpmm_hip_recommend.h): the header compiles as C, its functions are bound,
exported and built from csrc/recommend.hip; the numpy reference (tests/tools/recommend_ref.py) on a case computed by hand;
`Predictor.recommend` over a stand-in worker around tests/fake_worker.py that keeps a numpy table: the refusals, the slab walk with the
short slab's first rows copied, the table re-formed after `absorb_counts`."""
import importlib
import os
import re
import subprocess
import types

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package
from tools import overlap_ref
from tools import recommend_ref as RR
import test_countstats_cpu as CS
import test_rank_cpu as R

HEADER = os.path.join(ROOT, "include", "dpmm_hip_recommend.h")
FUNCS = ["dpmm_recommend_points", "dpmm_recommend_points_device", "dpmm_set_recommend"]
D, K = CS.D, CS.K


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
def test_header_compiles_as_c_and_is_bound_and_built(pkg, host, score):
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER])
    hdr = open(HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", body))) == FUNCS
    binding = importlib.import_module(pkg.__name__ + ".binding")
    assert sorted(n for n, _, _ in binding.ABI_RECOMMEND) == FUNCS
    assert "#define DPMM_RECOMMEND_MAX_TOP DPMM_SCORE_MAX_TOP" in hdr and binding.RECOMMEND_MAX_TOP == binding.SCORE_MAX_TOP == 16
    for name in ("set_recommend", "recommend_points_into"):
        assert callable(getattr(binding.Worker, name)), name
    csrc = os.path.join(ROOT, "dpmmsubclusters.jl_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "build/recommend.o" in re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "../../include/dpmm_hip_recommend.h" in re.search(r"^build/dpmm_api\.o:(.*)$", mk, flags=re.M).group(1).split()
    assert "DPMM_LAUNCH((recommend_kernel" in open(os.path.join(csrc, "recommend.hip")).read()      # the poison hook covers it
    assert host.Recommendation is score.Recommendation and host.recommend is score.recommend and callable(host.Predictor.recommend)
    assert score.Recommendation._fields == ("features", "prob", "labels", "skipped")


# ---------------------------------------------------------------------------------------------- the reference on a case computed by hand
def test_reference_on_a_hand_computed_case():
    # three clusters, six features; features 1 and 2 carry the same column: a tie in every mixture
    theta = np.array([[0.50, 0.125, 0.125, 0.25, 0.0, 0.0],
                      [0.00, 0.250, 0.250, 0.00, 0.5, 0.0],
                      [0.25, 0.125, 0.125, 0.00, 0.0, 0.5]])
    P = np.array([[1.0, 0.0, 0.0], [0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.25, 0.25, 0.5]], np.float32)
    r = RR.exact(P, theta)
    assert r.tolist() == [[0.5, 0.125, 0.125, 0.25, 0.0, 0.0], [0.25, 0.1875, 0.1875, 0.125, 0.25, 0.0], [0.125, 0.1875, 0.1875, 0.0, 0.25, 0.25],
                          [0.25, 0.15625, 0.15625, 0.0625, 0.125, 0.25]]
    assert RR.eps(3) == 5 * 2.0 ** -24
    seen = np.zeros((4, 6), bool)
    seen[0, 0] = True                      # point 0 holds its best feature
    seen[2, [0, 1, 3, 4]] = True           # point 2 has two candidates left: fewer than m
    f, v = RR.topm(r, seen, 3)
    assert f.tolist() == [[3, 1, 2], [0, 4, 1], [5, 2, -1], [0, 5, 1]] and f.dtype == np.int32
    assert v[0].tolist() == [0.25, 0.125, 0.125] and v[1].tolist() == [0.25, 0.25, 0.1875] and v[2, :2].tolist() == [0.25, 0.1875] and np.isnan(v[2, 2])
    f_all, _ = RR.topm(r, None, 3)
    assert f_all.tolist() == [[0, 3, 1], [0, 4, 1], [4, 5, 1], [0, 5, 1]]
    assert RR.check(f, v.astype(np.float32), P, theta, seen, 3) == 0.0
    assert RR.check(f_all, r[np.arange(4)[:, None], f_all].astype(np.float32), P, theta, None, 3) == 0.0
    # the checker refuses what the header forbids: a tie the wrong way round, a seen feature, a better candidate left out, a value off the bound
    wrong = f.copy()
    wrong[0, 1:] = [2, 1]
    with pytest.raises(AssertionError, match="equal bits"):
        RR.check(wrong, v.astype(np.float32), P, theta, seen, 3)
    wrong, wv = f.copy(), v.astype(np.float32)
    wrong[0], wv[0] = [0, 1, 2], [0.5, 0.125, 0.125]
    with pytest.raises(AssertionError, match="seen"):
        RR.check(wrong, wv, P, theta, seen, 3)
    with pytest.raises(AssertionError, match="left out"):
        RR.check(np.array([[3, 4, 5]] + f[1:].tolist(), np.int32), np.array([[0.25, 0.0, 0.0]] + v[1:].tolist(), np.float32), P, theta, seen, 3)
    off = v.astype(np.float32)
    off[1, 2] = np.float32(0.1875) * np.float32(1 + 2.0 ** -20)
    with pytest.raises(AssertionError, match="bound"):
        RR.check(f, off, P, theta, seen, 3)
    sk = np.array([False, True, False, False])
    g, w = f.copy(), v.astype(np.float32)
    g[1], w[1] = -1, np.nan
    RR.check(g, w, P, theta, seen, 3, skip_rows=sk)


# ---------------------------------------------------------------------------------------------- Predictor.recommend over a stand-in
class RecWorker(CS.CountWorker):
    """The table-keeping Multinomial stand-in (tests/fake_worker.py underneath) with the two calls `Predictor.recommend` makes, answered by
    tests/tools/recommend_ref.py from the Float32 image of the table it was handed."""

    def set_predictive_mult(self, logp, weights):
        super().set_predictive_mult(logp, weights)
        self.theta32 = None                                                      # a later set_predictive_* invalidates the table

    def set_recommend(self, theta):
        theta = np.asarray(theta)
        assert theta.dtype == np.float64 and theta.shape == (self.K, self.D)
        self.theta32 = theta.astype(np.float32)
        self.rec_sets = getattr(self, "rec_sets", []) + [theta.copy()]

    def recommend_points_into(self, views, m, exclude_seen=True):
        assert self.theta32 is not None, "DPMM_ESTATE: needs dpmm_set_recommend"
        self.rec_calls = getattr(self, "rec_calls", []) + [(int(m), bool(exclude_seen))]
        P, lab, part = overlap_ref.probs(self.table())
        r = (P.astype(np.float64) @ self.theta32.astype(np.float64)).astype(np.float32)
        f, v = RR.topm(r, (self.X != 0) if exclude_seen else None, m)
        f[~part], v[~part] = -1, np.nan
        assert views["features"].shape == (self.n, m) and views["prob"].shape == (self.n, m) and views["labels"].shape == (self.n,)
        views["features"][:], views["prob"][:], views["labels"][:] = f, v, lab
        return int((~part).sum())


N = 29


def open_mult(score, cap, **kw):
    return CS.open_mult(score, cap, factory=RecWorker, **kw)


def whole(p, X, m, exclude=True):
    """What one worker holding all the points answers."""
    w = RecWorker(1, X.shape[0], X.shape[1])
    w.logp, w.logw, w.K = p._wk.logp, p._wk.logw, p._wk.K
    w.theta32 = RR.theta_of(p.post["alpha"]).astype(np.float32)
    w.upload_points(np.ascontiguousarray(X.T))
    views = dict(features=np.empty((X.shape[1], m), np.int32), prob=np.empty((X.shape[1], m), np.float32), labels=np.empty(X.shape[1], np.int64))
    sk = w.recommend_points_into(views, m, exclude)
    return views, sk


@pytest.mark.parametrize("cap", [1, 7, N, N + 5])
def test_predictor_recommend_walks_the_slabs(score, cap):
    X = CS.counts(N, 5)
    X[1, 11] = np.nan                                                            # a NaN row of the table: skipped
    X[:, 3] = 1.0                                                                # a point that holds every feature: no candidates
    with open_mult(score, cap) as p:
        wk = p._wk
        for m, exclude in ((2, True), (D, True), (3, False)):
            want, sk = whole(p, X, m, exclude)
            got = p.recommend(X, m, exclude_seen=exclude)
            assert isinstance(got, score.Recommendation) and isinstance(got.skipped, int)
            assert got.features.shape == (N, m) and got.features.dtype == np.int32 and got.prob.dtype == np.float32 and got.labels.dtype == np.int64
            assert np.array_equal(got.features, want["features"]) and got.prob.tobytes() == want["prob"].tobytes()      # the short slab's first rows
            assert np.array_equal(got.labels, want["labels"])
            assert got.skipped == sk == 1 and (got.features[11] == -1).all() and np.isnan(got.prob[11]).all()       # the padding is not counted
            if exclude:
                assert (got.features[3] == -1).all()
        assert all(u == cap for u in wk.uploads)                                 # never a short upload
        assert wk.rec_calls[:-(-N // cap)] == [(2, True)] * -(-N // cap)
        assert len(wk.rec_sets) == 1                                             # the table is formed once
        assert wk.rec_sets[0].tobytes() == RR.theta_of(p.post["alpha"]).tobytes() == p.sampler_tables()[1].tobytes()
        e = p.recommend(X[:, :0], 2)
        assert e.features.shape == (0, 2) and e.prob.shape == (0, 2) and e.labels.shape == (0,) and e.skipped == 0


def test_refusals(score):
    X = CS.counts(10, 6)
    with open_mult(score, 8) as p:
        for m in (0, -1, D + 1, 17):
            with pytest.raises(ValueError, match=f"1..{D}"):
                p.recommend(X, m)
        with pytest.raises(ValueError, match="dimension"):
            p.recommend(np.zeros((D + 1, 5), np.float32), 2)
        assert not hasattr(p._wk, "rec_calls")                                   # refused before the worker was asked
    with pytest.raises(RuntimeError, match="closed"):
        p.recommend(X, 2)
    wide = score.Predictor.__new__(score.Predictor)
    a = np.ones((2, 40), np.float32)
    wide._setup(1, 40, 10.0, np.full(2, 20.0), dict(alpha=a), 8, 0, RecWorker)
    with wide:
        with pytest.raises(ValueError, match="1..16"):                           # min(D, 16)
            wide.recommend(np.zeros((40, 3), np.float32), 17)
        assert wide.recommend(np.zeros((40, 3), np.float32), 16).features.shape == (3, 16)
    made = []

    class NiwWorker(RecWorker):
        def set_predictive_niw(self, *a):
            made.append(self)
    with score.Predictor(R.model(3, K), capacity=16, worker_factory=NiwWorker) as niw:
        with pytest.raises(ValueError, match="regressor"):
            niw.recommend(np.ones((3, 4), np.float32), 1)
        assert made and not hasattr(made[0], "rec_calls")

    class Cannot(CS.CountWorker):                                                # a worker without the call
        pass
    with CS.open_mult(score, 8, factory=Cannot) as p:
        with pytest.raises(RuntimeError, match="dpmm_recommend_points"):
            p.recommend(X, 2)


def test_one_shot_and_the_table_is_reformed_after_absorb_counts(score, host):
    X = CS.counts(60, 8)
    Y = CS.counts(20, 9)
    with open_mult(score, 16) as p:
        wk = p._wk
        before = p.recommend(Y, 3)
        assert p._recommend_set and len(wk.rec_sets) == 1
        p.absorb_counts(X, assign="soft")
        assert not p._recommend_set and wk.theta32 is None                       # the worker's table went with the reload
        after = p.recommend(Y, 3)
        assert len(wk.rec_sets) == 2 and wk.rec_sets[1].tobytes() == RR.theta_of(p.post["alpha"]).tobytes()
        assert wk.rec_sets[1].tobytes() != wk.rec_sets[0].tobytes() and after.prob.tobytes() != before.prob.tobytes()
        with CS.open_mult(score, 16, factory=RecWorker, post=p.post, count=p.points_count) as fresh:
            want = fresh.recommend(Y, 3)
        assert np.array_equal(after.features, want.features) and after.prob.tobytes() == want.prob.tobytes() and np.array_equal(after.labels, want.labels)
        p.recommend(Y, 3)
        assert len(wk.rec_sets) == 2                                             # ... and only then
    s = types.SimpleNamespace(K=K, prior=types.SimpleNamespace(kind=1, dim=D), post=dict(alpha=np.repeat(CS.alpha_post()["alpha"], 3, axis=0)), alpha=10.0,
                              points_count=np.full(K, 20), wk=types.SimpleNamespace(device=0))
    n_made = len(R.TableWorker.made)
    one = host.recommend(types.SimpleNamespace(sampler=s), Y, 3, capacity=16, worker_factory=RecWorker, exclude_seen=False)
    assert len(R.TableWorker.made) == n_made + 1 and R.TableWorker.made[-1].closed      # the one-shot call closes its worker
    with open_mult(score, 64) as q:
        two = q.recommend(Y, 3, exclude_seen=False)
    assert np.array_equal(one.features, two.features) and one.prob.tobytes() == two.prob.tobytes()
