"""CPU-side checks of host/score.py's Predictor (slab loop, padding, lengths, errors, save / load) with a stand-in worker defined here,
and of the boundary of include/dpmm_hip_score.h: the header compiles as C, its functions are bound and exported."""
import ctypes
import importlib
import os
import re
import subprocess
import types

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


class StandIn:
    """Records what a Predictor hands its worker; scores with plain numpy: a_k(i) = log w_k - |x_i - c_k|^2 with c_k a function of the
    predictive parameters, so that labels, probabilities and log-density are per-point functions of the point alone."""
    made = []

    def __init__(self, prior, D, n_local, first_index=0, device=0, seed=0):
        self.prior, self.D, self.n, self.device = prior, D, n_local, device
        self.uploads, self.predictive_calls, self.closed = [], 0, False
        StandIn.made.append(self)

    def close(self):
        self.closed = True

    def upload_points(self, X):
        X = np.asarray(X)
        assert X.shape == (self.n, self.D) and X.dtype == np.float32, (X.shape, X.dtype)      # never a short upload
        self.X = X.copy()
        self.uploads.append(X.shape[0])

    def set_predictive_niw(self, m, R, logdet, df, weights):
        self.predictive_calls += 1
        self.centres, self.logw, self.K = np.asarray(m, np.float64), np.log(np.asarray(weights, np.float64)), len(weights)

    def set_predictive_mult(self, logp, weights):
        self.predictive_calls += 1
        self.centres, self.logw, self.K = np.asarray(logp, np.float64), np.log(np.asarray(weights, np.float64)), len(weights)

    def score_points_into(self, outs, m=0):
        a = self.logw[None, :] - ((self.X[:, None, :].astype(np.float64) - self.centres[None, :, :]) ** 2).sum(-1)      # (n, K)
        M = a.max(1, keepdims=True)
        e = np.exp(a - M)
        p = (e / e.sum(1, keepdims=True)).astype(np.float32)
        full = dict(labels=a.argmax(1) + 1, logdens=(M[:, 0] + np.log(e.sum(1))).astype(np.float32), probs=p)
        order = np.argsort(-p, axis=1, kind="stable")[:, :m]
        full["top_idx"], full["top_prob"] = order + 1, np.take_along_axis(p, order, axis=1)
        for name, arr in outs.items():
            assert arr.shape[0] == self.n, (name, arr.shape)
            arr[...] = full[name]


def model(kind, D, K, seed=0):
    """What a Predictor reads of a fitted model."""
    rng = np.random.default_rng(seed)
    if kind == 0:
        A = rng.standard_normal((3 * K, D, D)) * 0.1 + np.eye(D)
        post = dict(kappa=1 + rng.random(3 * K), nu=D + 3 + rng.random(3 * K), m=rng.standard_normal((3 * K, D)), U=np.triu(A) + 2 * np.eye(D),
                    logdet_psi=np.zeros(3 * K))
    else:
        post = dict(alpha=(1 + rng.random((3 * K, D))).astype(np.float32))
    prior = types.SimpleNamespace(kind=kind, dim=D)
    s = types.SimpleNamespace(K=K, prior=prior, post=post, alpha=10.0, points_count=rng.integers(5, 50, K), wk=types.SimpleNamespace(device=0))
    return types.SimpleNamespace(sampler=s)


def direct(p, X):
    """The stand-in's scores of all points at once: what the slab loop must reproduce."""
    wk = StandIn(p.kind, p.D, X.shape[1])
    wk.centres, wk.logw, wk.K = p._wk.centres, p._wk.logw, p._wk.K
    wk.upload_points(np.ascontiguousarray(X.T, dtype=np.float32))
    return wk


@pytest.mark.parametrize("n", [0, 1, 9, 10, 11, 20, 37])
def test_slab_loop_padding_and_lengths(score, n):
    D, K, cap = 3, 4, 10
    p = score.Predictor(model(0, D, K), capacity=cap, worker_factory=StandIn)
    wk = p._wk
    assert wk.n == cap and wk.predictive_calls == 1
    X = np.random.default_rng(n).standard_normal((D, n))
    lab, probs = p.predict(X)
    assert lab.shape == (n,) and lab.dtype == np.int64 and probs.shape == (n, K) and probs.dtype == np.float32
    assert wk.uploads == [cap] * -(-n // cap)                      # ceil(n / cap) uploads, every one of `capacity` points
    if n % cap:
        assert np.all(wk.X[n % cap:] == 0) and np.array_equal(wk.X[:n % cap], X[:, n - n % cap:].T.astype(np.float32))
    l2, idx, tp = p.predict_topk(X, 2)
    ld = p.score_samples(X)
    assert idx.shape == (n, 2) and idx.dtype == np.int64 and tp.shape == (n, 2) and ld.shape == (n,) and ld.dtype == np.float32
    assert p.predict_labels(X).shape == (n,)
    assert wk.predictive_calls == 1 and len(StandIn.made) >= 1     # parameters loaded once, one worker
    if n:
        ref = direct(p, X)
        outs = dict(labels=np.empty(n, np.int64), logdens=np.empty(n, np.float32), probs=np.empty((n, K), np.float32),
                    top_idx=np.empty((n, 2), np.int64), top_prob=np.empty((n, 2), np.float32))
        ref.score_points_into(outs, m=2)
        assert np.array_equal(lab, outs["labels"]) and np.array_equal(l2, outs["labels"]) and np.array_equal(probs, outs["probs"])
        assert np.array_equal(idx, outs["top_idx"]) and np.array_equal(tp, outs["top_prob"]) and np.array_equal(ld, outs["logdens"])
    p.close()
    assert wk.closed
    with pytest.raises(RuntimeError):
        p.predict(X)


def test_one_worker_serves_every_call_and_the_context_manager_closes_it(score):
    before = len(StandIn.made)
    with score.Predictor(model(0, 2, 3), capacity=8, worker_factory=StandIn) as p:
        for n in (3, 8, 30):
            assert p.predict_labels(np.zeros((2, n))).shape == (n,)
        wk = p._wk
    assert len(StandIn.made) == before + 1 and wk.closed and wk.predictive_calls == 1


def test_errors(score, monkeypatch):
    p = score.Predictor(model(0, 3, 4), capacity=10, worker_factory=StandIn)
    with pytest.raises(ValueError, match="dimension"):
        p.predict(np.zeros((4, 5)))
    with pytest.raises(ValueError):
        p.predict_topk(np.zeros((3, 5)), 0)
    with pytest.raises(ValueError):
        p.predict_topk(np.zeros((3, 5)), 5)                          # K = 4
    sparse = (np.array([0, 1, 2]), np.array([0, 1]), np.array([1.0, 2.0], np.float32), (3, 2))
    with pytest.raises(TypeError, match="Multinomial"):
        p.predict(sparse)
    # a tensor on another device than the Predictor's, and a `device=` that disagrees with the tensor's
    fake = types.SimpleNamespace(device_index=1, torch_device="cuda:1", shape=(3, 5))
    monkeypatch.setattr(score._tensors, "as_device_points", lambda data: fake)
    with pytest.raises(ValueError, match="device"):
        p.predict(object())
    p.close()
    q = score.Predictor(model(0, 3, 4), capacity=10, device=1, worker_factory=StandIn)
    fake.device_index = 0
    with pytest.raises(ValueError, match="disagrees"):
        q.predict(object())
    q.close()
    with pytest.raises(ValueError):
        score.Predictor(model(0, 3, 4), capacity=0, worker_factory=StandIn)


def test_sparse_columns_through_a_multinomial_predictor(score):
    D, K, cap, n = 6, 3, 4, 9
    rng = np.random.default_rng(2)
    X = rng.poisson(0.7, (D, n)).astype(np.float32)
    cp = np.concatenate([[0], np.cumsum((X != 0).sum(0))]).astype(np.int64)
    rv = np.concatenate([np.flatnonzero(X[:, i]) for i in range(n)]).astype(np.int64)
    nz = np.concatenate([X[X[:, i] != 0, i] for i in range(n)]).astype(np.float32)
    with score.Predictor(model(1, D, K), capacity=cap, worker_factory=StandIn) as p:
        a = p.predict((cp, rv, nz, (D, n)))
        b = p.predict(X)
        assert p._wk.uploads == [cap] * 6
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("kind", [0, 1])
def test_save_load_round_trip(score, tmp_path, kind):
    D, K = 3, 4
    p = score.Predictor(model(kind, D, K, seed=5), capacity=7, worker_factory=StandIn)
    path = str(tmp_path / "model.npz")
    p.save(path)
    q = score.Predictor.load(path, capacity=5, worker_factory=StandIn)
    assert (q.kind, q.D, q.K, q.alpha) == (p.kind, p.D, p.K, p.alpha) and np.array_equal(q.points_count, p.points_count)
    assert sorted(q.post) == sorted(p.post) and all(np.array_equal(q.post[k], p.post[k]) for k in p.post)
    assert all(v.shape[0] == K for v in q.post.values())             # the K clusters' rows only
    assert np.array_equal(q._wk.centres, p._wk.centres) and np.array_equal(q._wk.logw, p._wk.logw)
    X = np.random.default_rng(1).random((D, 12))
    assert np.array_equal(p.predict(X)[1], q.predict(X)[1])
    with np.load(path) as z:
        assert {"kind", "D", "alpha", "points_count"} <= set(z.files)
    p.close(); q.close()


def test_module_level_conveniences(score):
    m = model(0, 2, 3)
    X = np.random.default_rng(3).standard_normal((2, 25))
    before = len(StandIn.made)
    ld = score.score_samples(m, X, capacity=8, worker_factory=StandIn)
    lab, idx, tp = score.predict_topk(m, X, 2, capacity=8, worker_factory=StandIn)
    assert ld.shape == (25,) and idx.shape == (25, 2) and tp.shape == (25, 2) and lab.shape == (25,)
    assert len(StandIn.made) == before + 2 and all(w.closed for w in StandIn.made[before:])
    host = importlib.import_module(score.__name__.rsplit(".", 1)[0])
    assert host.Predictor is score.Predictor and host.score_samples is score.score_samples and host.predict_topk is score.predict_topk


# ---------------------------------------------------------------------------------------------- the C boundary
def declared():
    src = open(os.path.join(ROOT, "include", "dpmm_hip_score.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", src)))


def test_header_compiles_as_c_and_is_bound_and_exported(pkg):
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "dpmm_hip_score.h")])
    binding = importlib.import_module(pkg.__name__ + ".binding")
    names = declared()
    assert names == sorted(n for n, _, _ in binding.ABI_SCORE) == ["dpmm_score_points", "dpmm_score_points_device"]
    assert not set(names) & set(n for n, _, _ in binding.ABI + binding.ABI_TENSOR)
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for n in names:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                               # additive: the version stays
    hdr = open(os.path.join(ROOT, "include", "dpmm_hip_score.h")).read()
    assert int(re.search(r"#define DPMM_OPT_SCORE_TABLE_MB (\d+)", hdr).group(1)) == binding.OPT_SCORE_TABLE_MB
    assert int(re.search(r"#define DPMM_SCORE_MAX_TOP (\d+)", hdr).group(1)) == binding.SCORE_MAX_TOP
    # the struct the binding passes has the header's members in the header's order
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    struct = body[body.index("typedef struct {"):body.index("} dpmm_score_out;")]
    assert re.findall(r"\*?\s*([a-z_]+);", struct) == [f[0] for f in binding.ScoreOut._fields_]
