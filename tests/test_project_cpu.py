"""CPU-side checks of host/project.py (PCA from a subsample, random bases, save / load, argument errors), of the `project=` keyword's
refusals, of the Predictor's plumbing with a stand-in worker whose projected entry points are numpy Float64, and of the boundary of
include/dpmm_hip_project.h: the header compiles as C, its functions are bound and exported."""
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
def host(pkg):
    return importlib.import_module(pkg.__name__ + ".host")


@pytest.fixture(scope="module")
def project(pkg):
    return importlib.import_module(pkg.__name__ + ".host.project")


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


class StandIn:
    """A worker that scores with plain numpy (a_k(i) = log w_k - |y_i - c_k|^2) and projects in Float64: y = (x - mu)' W, rounded once."""
    made = []

    def __init__(self, prior, D, n_local, first_index=0, device=0, seed=0):
        self.prior, self.D, self.n, self.device = prior, D, n_local, device
        self.W = self.mu = None
        self.plain = self.projected = 0
        StandIn.made.append(self)

    def close(self):
        pass

    def upload_points(self, X):
        X = np.asarray(X)
        assert X.shape == (self.n, self.D) and X.dtype == np.float32, (X.shape, X.dtype)
        self.X = X.copy()
        self.plain += 1

    def set_projection(self, W, mu=None):
        W = np.asarray(W, np.float64)
        assert W.ndim == 2 and W.shape[1] == self.D
        self.W, self.mu = W, np.zeros(W.shape[0]) if mu is None else np.asarray(mu, np.float64)

    def clear_projection(self):
        self.W = self.mu = None

    def upload_points_projected(self, X):
        X = np.asarray(X)
        assert self.W is not None and X.dtype == np.float32 and X.shape == (self.n, self.W.shape[0]), (X.shape, X.dtype)
        self.X = (X.astype(np.float64) @ self.W - self.mu @ self.W).astype(np.float32)
        self.projected += 1

    def get_points(self):
        return self.X.copy()

    def set_predictive_niw(self, m, R, logdet, df, weights):
        self.centres, self.logw, self.K = np.asarray(m, np.float64), np.log(np.asarray(weights, np.float64)), len(weights)

    def score_points_into(self, outs, m=0):
        a = self.logw[None, :] - ((self.X[:, None, :].astype(np.float64) - self.centres[None, :, :]) ** 2).sum(-1)
        M = a.max(1, keepdims=True)
        e = np.exp(a - M)
        p = (e / e.sum(1, keepdims=True)).astype(np.float32)
        full = dict(labels=a.argmax(1) + 1, logdens=(M[:, 0] + np.log(e.sum(1))).astype(np.float32), probs=p)
        order = np.argsort(-p, axis=1, kind="stable")[:, :m]
        full["top_idx"], full["top_prob"] = order + 1, np.take_along_axis(p, order, axis=1)
        for name, arr in outs.items():
            assert arr.shape[0] == self.n, (name, arr.shape)
            arr[...] = full[name]


def model(D, K, projection=None, seed=0):
    """What a Predictor reads of a fitted NIW model."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((3 * K, D, D)) * 0.1 + np.eye(D)
    post = dict(kappa=1 + rng.random(3 * K), nu=D + 3 + rng.random(3 * K), m=rng.standard_normal((3 * K, D)), U=np.triu(A) + 2 * np.eye(D),
                logdet_psi=np.zeros(3 * K))
    s = types.SimpleNamespace(K=K, prior=types.SimpleNamespace(kind=0, dim=D), post=post, alpha=10.0, points_count=rng.integers(5, 50, K),
                              wk=types.SimpleNamespace(device=0))
    return types.SimpleNamespace(sampler=s, projection=projection)


# ---- PCA
D_IN, N, RANK = 96, 4000, 5


@pytest.fixture(scope="module")
def lowrank():
    rng = np.random.default_rng(11)
    U, _ = np.linalg.qr(rng.standard_normal((D_IN, RANK)))
    V, _ = np.linalg.qr(rng.standard_normal((N, RANK)))
    X = (U * np.array([10.0, 8.0, 6.0, 4.0, 3.0])) @ V.T * np.sqrt(N) + 0.01 * rng.standard_normal((D_IN, N)) + rng.standard_normal((D_IN, 1))
    X.setflags(write=False)
    return X


def test_pca_recovers_the_subspace_of_the_float64_svd(project, lowrank):
    X = lowrank
    P = project.fit_projection(X, RANK, sample=N)
    assert (P.D_in, P.d) == (D_IN, RANK) and P.basis.dtype == np.float64 and P.mean.dtype == np.float64
    Xc = X - X.mean(1, keepdims=True)
    Uref = np.linalg.svd(Xc, full_matrices=False)[0][:, :RANK]
    cosines = np.linalg.svd(Uref.T @ P.basis, compute_uv=False)
    print("smallest cosine of the principal angles: 1 - %.3e" % (1 - cosines.min()))
    assert cosines.min() >= 1 - 1e-9
    assert np.abs(P.basis.T @ P.basis - np.eye(RANK)).max() <= 1e-12
    assert np.abs(P.mean - X.mean(1)).max() <= 1e-12
    top = P.basis[np.abs(P.basis).argmax(0), np.arange(RANK)]
    assert (top > 0).all()                                                    # the sign convention
    assert (np.diff(P.explained_variance) <= 0).all()
    with pytest.raises((ValueError, AttributeError)):
        P.basis[0, 0] = 1.0                                                   # immutable
    with pytest.raises(AttributeError):
        P.mean = None


def test_pca_same_bits_from_numpy_and_from_a_strided_torch_view(project, lowrank):
    import torch
    P = project.fit_projection(lowrank, RANK, sample=N)
    big = torch.zeros((N, 2 * D_IN), dtype=torch.float64)
    big[:, ::2] = torch.from_numpy(lowrank.copy()).T
    view = big[:, ::2].T                                                      # (D_IN, N), strides (2, 2 D_IN)
    assert not view.is_contiguous()
    Q = project.fit_projection(view, RANK, sample=N)
    assert P.basis.tobytes() == Q.basis.tobytes() and P.mean.tobytes() == Q.mean.tobytes()
    # a subsample: the indices are a function of the seed, and sorted
    a, b, c = (project.fit_projection(lowrank, 3, sample=500, seed=s) for s in (4, 4, 5))
    assert a.basis.tobytes() == b.basis.tobytes() and a.basis.tobytes() != c.basis.tobytes()


def test_whitening_gives_unit_sample_variances(project, lowrank):
    P = project.fit_projection(lowrank, RANK, sample=N, whiten=True)
    Y = P.basis.T @ (lowrank - P.mean[:, None])
    assert np.abs(Y.var(1, ddof=1) - 1).max() <= 1e-9
    flat = np.zeros((8, 50)); flat[0] = np.arange(50)
    with pytest.raises(ValueError):
        project.fit_projection(flat, 3, whiten=True)


def test_random_projection_is_orthonormal_and_reproducible(project):
    P, Q, R = project.random_projection(300, 17, seed=3), project.random_projection(300, 17, seed=3), project.random_projection(300, 17, seed=4)
    assert np.abs(P.basis.T @ P.basis - np.eye(17)).max() <= 1e-12
    assert P.basis.tobytes() == Q.basis.tobytes() and P.basis.tobytes() != R.basis.tobytes()
    assert (P.basis[np.abs(P.basis).argmax(0), np.arange(17)] > 0).all() and not P.mean.any()
    assert np.array_equal(project.random_projection(5, 2, mean=np.arange(5.0)).mean, np.arange(5.0))


def test_projection_save_load_round_trip(project, tmp_path, lowrank):
    P = project.fit_projection(lowrank, 4, sample=1000, seed=2)
    path = str(tmp_path / "p.npz")
    P.save(path)
    Q = project.Projection.load(path)
    assert all(getattr(P, k).tobytes() == getattr(Q, k).tobytes() for k in ("mean", "basis", "explained_variance"))
    R = project.random_projection(7, 2)
    R.save(path)
    assert project.Projection.load(path).explained_variance is None


def test_argument_errors(project, host):
    X = np.zeros((300, 10))
    with pytest.raises(ValueError):
        project.fit_projection(np.zeros((300, 10)), 257)                      # d > 256
    with pytest.raises(ValueError):
        project.fit_projection(np.zeros((8, 10)), 9)                          # d > D_in
    with pytest.raises(ValueError):
        project.fit_projection(np.zeros((4097, 2)), 2)                        # D_in > 4096
    with pytest.raises(ValueError):
        project.random_projection(4097, 2)
    with pytest.raises(ValueError):
        project.fit_projection(X, 0)
    with pytest.raises(ValueError):
        project.Projection(np.zeros(3), np.zeros((4, 2)))
    P = project.random_projection(300, 4)
    with pytest.raises(TypeError):                                            # a Multinomial prior
        host.fit(np.ones((300, 10)), host.multinomial_hyper(np.ones(4)), 1.0, project=P, iters=1, verbose=False, worker_factory=StandIn)
    two = types.SimpleNamespace(world=2, rank=0, device=0)
    with pytest.raises(ValueError, match="more than one rank"):               # an int with two ranks: no agreed way to share a fitted basis
        host.fit(X, 1.0, project=4, iters=1, verbose=False, comm=two, worker_factory=StandIn)
    with pytest.raises(TypeError):
        host.fit(X, 1.0, project="pca", iters=1, verbose=False, worker_factory=StandIn)
    with pytest.raises(ValueError):                                           # data that the projection does not read
        host.fit(np.zeros((299, 10)), 1.0, project=P, iters=1, verbose=False, worker_factory=StandIn)


# ---- Predictor plumbing
def test_predictor_projects_raw_data_and_takes_projected_data_as_it_is(project, score, tmp_path):
    D_in, d, K, cap, n = 40, 3, 4, 10, 37
    P = project.random_projection(D_in, d, seed=1, mean=np.linspace(-1, 1, D_in))
    X = np.random.default_rng(3).standard_normal((D_in, n)).astype(np.float32)
    Y = P.transform(X, capacity=16, worker_factory=StandIn)
    assert Y.shape == (d, n) and Y.dtype == np.float32
    assert np.array_equal(Y, ((X.T.astype(np.float64) @ P.basis - P.mean @ P.basis).astype(np.float32)).T)
    with pytest.raises(ValueError):
        P.transform(X[:-1], worker_factory=StandIn)
    p = score.Predictor(model(d, K, P), capacity=cap, worker_factory=StandIn)
    assert p.projection is P and p._wk.W is not None
    for call in (lambda q, Z: q.predict(Z), lambda q, Z: q.predict_topk(Z, 2), lambda q, Z: (q.score_samples(Z),), lambda q, Z: (q.predict_labels(Z),)):
        for a, b in zip(call(p, X), call(p, Y)):
            assert np.array_equal(a, b)
    assert p._wk.projected == 4 * 4 and p._wk.plain == 4 * 4                  # every slab, the short one included, through its own entry point
    with pytest.raises(ValueError):
        p.predict(X[:7])                                                      # neither D_in nor d rows
    path = str(tmp_path / "m.npz")
    p.save(path)
    q = score.Predictor.load(path, capacity=7, worker_factory=StandIn)
    assert q.projection is not None and q.projection.basis.tobytes() == P.basis.tobytes() and q.projection.mean.tobytes() == P.mean.tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(q.predict(X), p.predict(Y)))
    # a model without one: saved and loaded as ever, D_in-row data refused
    r = score.Predictor(model(d, K), capacity=cap, worker_factory=StandIn)
    r.save(path)
    with np.load(path) as z:
        assert not [k for k in z.files if k.startswith("proj_")]
    t = score.Predictor.load(path, capacity=cap, worker_factory=StandIn)
    assert t.projection is None and all(np.array_equal(a, b) for a, b in zip(t.predict(Y), p.predict(Y)))
    with pytest.raises(ValueError):
        t.predict(X)


# ---- the header
def test_header_compiles_as_c_and_is_bound_and_exported(pkg):
    hdr = os.path.join(ROOT, "include", "dpmm_hip_project.h")
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", hdr])
    binding = importlib.import_module(pkg.__name__ + ".binding")
    src = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(dpmm_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(n for n, _, _ in binding.ABI_PROJECT) == ["dpmm_set_projection", "dpmm_upload_points_projected", "dpmm_upload_points_projected_device"]
    assert not set(names) & set(n for n, _, _ in binding.ABI + binding.ABI_TENSOR)
    assert int(re.search(r"#define DPMM_MAX_DIM_PROJECT_IN (\d+)", src).group(1)) == binding.MAX_DIM_PROJECT_IN == 4096
    pkg.build_library()
    lib = ctypes.CDLL(pkg.lib_path())
    for n in names:
        assert hasattr(lib, n), n
    lib.dpmm_abi_version.restype = ctypes.c_int
    assert lib.dpmm_abi_version() == 3                                        # additive: the version stays
    for m in ("set_projection", "clear_projection", "upload_points_projected", "upload_points_projected_strided_device", "upload_points_projected_tensor"):
        assert callable(getattr(binding.Worker, m))
