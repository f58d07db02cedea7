"""The lean kernel's norm certificate (DPMM_OPT_LEAN_NORM_CERT, csrc/niw_lean.hip): a tile whose points lie within r of mu_k0 has
a_k0(x) >= c0 - (sn2_k0 r)^2 / 2; where the pair-ball test with that threshold excludes every other cluster the tile is settled without the
reference bracket.  Labels and sub-labels must be those of the kernel path without it, bit for bit; every tile it settles must be one that a
Float64 evaluation clears; sn2 must be a certified norm bound, never above sn, from both of its producers."""
import importlib

import numpy as np
import pytest

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

MARGIN = 50.0        # the library's default screen margin
SD_FAR, SD_EDGE, SD_CLOSE = 10.0, 6.0, 0.4     # separations (a), (b), (c).  (b) from a numpy model of the certificate on these problems (norm bound
                                               # 1.06 x, radius of every 64-point tile): D = 64, K = 32: 3 of 128 tiles settled at sd 4, 52 at sd 6, 83 at sd 10;
                                               # D = 36, K = 65: 0 of 260 at sd 4, 58 at sd 6, 165 at sd 10; at sd 6 also
                                               # D = 36, K = 32: 35 of 128; D = 64, K = 65: 63 of 260; K = 256: 216 (D = 64) and 136 (D = 36) of 1024


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def pb_maxk():
    from dpmmsubclusters_jl_amd import binding
    return binding.PB_MAXK


_PROBLEMS = {}


def problem(D, K, sd):
    """K components with covariances InvWishart(D + 2, I) (as the bench generator draws them), means N(0, sd^2 I), n = 64 * 3 * K + 17 points in
    component order (every bin ends in a partly filled tile); the sub-clusters share the component's covariance, their means sit a little apart.
    The parameters are the Float32 values the worker is given: the upper-triangular factors R (R' R = Sigma^-1) go in as they are."""
    key = (D, K, sd)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    rng = np.random.default_rng(1000 * D + 10 * K + int(10 * sd))
    n = 64 * 3 * K + 17
    mu = np.zeros((3 * K, D), np.float32); R = np.zeros((3 * K, D, D), np.float32); logdet = np.zeros(3 * K, np.float32)
    z = np.minimum(np.arange(n) // (n // K), K - 1)
    X = np.empty((n, D), np.float32)
    for k in range(K):
        G = rng.normal(size=(D, D + 2))
        C = np.linalg.cholesky(G @ G.T)                         # Sigma^-1 = C C' ~ Wishart(D + 2, I): R = C'
        m = rng.normal(size=D) * sd
        off = np.linalg.solve(C.T, rng.normal(size=D)) * 0.3
        mu[3 * k], mu[3 * k + 1], mu[3 * k + 2] = m, m + off, m - off
        R[3 * k:3 * k + 3] = C.T
        logdet[3 * k:3 * k + 3] = -2.0 * np.log(np.diag(C)).sum()
        idx = np.nonzero(z == k)[0]
        X[idx] = (m + np.linalg.solve(C.T, rng.normal(size=(D, len(idx)))).T).astype(np.float32)
    P = dict(D=D, K=K, n=n, X=X, z=z, mu=mu, R=R, logdet=logdet, lr=np.full((K, 2), 0.5, np.float32), w=np.full(K, 1.0 / K, np.float32))
    _PROBLEMS[key] = P
    return P


def loglik64(P, X):
    """a_j(x) = cst_j - |R_j (x - mu_j)|^2 / 2 for every point and cluster, in Float64 from the Float32 parameters the worker holds."""
    D, K = P["D"], P["K"]
    mu = P["mu"][0::3].astype(np.float64); R = P["R"][0::3].astype(np.float64)
    cst = -0.5 * P["logdet"][0::3].astype(np.float64) + np.log(P["w"].astype(np.float64))
    X = X.astype(np.float64)
    a = np.empty((len(X), K))
    for j in range(K):
        y = (X - mu[j]) @ R[j].T
        a[:, j] = cst[j] - 0.5 * (y * y).sum(1)
    return a


def run(pkg, P, cert, X=None):
    """Two sweeps from fixed parameters (the second on the kernel's own labels).  Returns the labels and sub-labels after each, the work counters of
    both, sn, sn2 and, per sweep, (labels before the sweep, flags of the points whose tile the certificate settled)."""
    from dpmmsubclusters_jl_amd import binding
    D, K, n = P["D"], P["K"], P["n"]
    wk = pkg.Worker(pkg.PRIOR_NIW, D, n, first_index=0, device=0, seed=41)
    wk.upload_points(P["X"] if X is None else X)
    wk.set_option(binding.OPT_LEAN_NORM_CERT, cert)               # (2: the tight sn2 whatever the size -- these problems are far below the size at which 1 writes it)
    if K > 64:
        wk.set_option(binding.OPT_PRESCREEN, 0)
    par = (P["mu"], P["R"], P["logdet"], P["lr"], P["w"])
    wk.set_params_niw_chol(*par)
    wk.set_labels(P["z"] + 1, 1 + (np.arange(n) & 1))
    wk.suffstats_packed(None)                                  # the bin-sorted visiting order
    wk.set_params_niw_chol(*par)
    _, sn = wk.debug_pair_ball()
    sn2 = wk.debug_pair_ball_sn2()
    wk.last_sweep_work()
    wk.debug_norm_cert_points(enable=True, read=False)
    labs, settled = [], []
    before = P["z"] + 1
    for ep in (1, 2):
        wk.sweep(ep)
        labs.append(wk.get_labels())
        settled.append((before, wk.debug_norm_cert_points(enable=True)))
        before = labs[-1][0]
        wk.suffstats_packed(None)
        wk.set_params_niw_chol(*par)
    work = wk.last_sweep_work()
    wk.close()
    return labs, work, sn, sn2, settled


def same(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def total(w, k):
    return round(w[k] * max(1, w["launches"]))                  # (the counters come back per launch)


def check_sound(P, X, settled):
    """Every point of a tile the certificate settled: a_j(x) < a_k0(x) - margin for all j != k0 (k0: the point's label before the sweep)."""
    a = loglik64(P, X)
    for before, flags in settled:
        i = np.nonzero(flags)[0]
        k0 = before[i] - 1
        own = a[i, k0]
        rest = a[i].copy()
        rest[np.arange(len(i)), k0] = -np.inf
        assert np.all(rest.max(axis=1) < own - MARGIN)


def check_sn2(sn, sn2, R32):
    true_s = np.linalg.norm(R32.astype(np.float64), 2, axis=(1, 2))      # sqrt(lambda_max(R' R)) of the Float32 factor the kernels hold
    print(f"   sn2 / |R|_2: {np.min(sn2 / true_s):.6f} .. {np.max(sn2 / true_s):.4f}; sn / |R|_2: max {np.max(sn / true_s):.4f}")
    assert np.all(sn2 >= true_s) and np.all(sn2 <= sn)
    assert np.all(sn2 <= 1.2 * true_s)                          # (three squarings: |.|_inf <= 8 |.|_2 of the eighth power -> 8^(1/16) = 1.14)


@pytest.mark.parametrize("D", [64, 36])
@pytest.mark.parametrize("K", [2, 32, 65, "PB_MAXK"])
@pytest.mark.parametrize("sd", [SD_FAR, SD_EDGE])
def test_settled_tiles_same_labels_and_sound(pkg, D, K, sd):
    """Separations (a) and (b): labels and sub-labels bit-identical with the option at 0 and 1; the certificate settles tiles (fewer brackets than
    tiles) and -- at (b), and wherever K > 2 at (a) -- leaves others to the bracket; the points of every settled tile are cleared by the Float64
    evaluation; sn2 >= sqrt(lambda_max(R' R)) in Float64 and sn2 <= sn for every cluster."""
    K = pb_maxk() if K == "PB_MAXK" else K
    P = problem(D, K, sd)
    l1, w1, sn, sn2, settled = run(pkg, P, 2)
    l0, w0, _, sn2_0, settled0 = run(pkg, P, 0)
    nset = [int(f.sum()) for _, f in settled]
    print(f"D={D} K={K} sd={sd}: tiles {total(w1, 'wave_tiles')} brackets {total(w1, 'brackets')} (option 0: {total(w0, 'brackets')}) "
          f"norm-certificate tiles {total(w1, 'norm_cert_tiles')}, their points per sweep {nset} of {P['n']}")
    assert same(l1, l0)
    assert np.array_equal(sn2_0, sn)                            # (option 0: the block is written, with the loose bound)
    assert total(w0, "norm_cert_tiles") == 0 and not any(f.any() for _, f in settled0)
    assert total(w1, "brackets") + total(w1, "norm_cert_tiles") == total(w0, "brackets")
    if sd == SD_FAR or K > 2:                                   # (K = 2 at (b): eight tiles, the model settles 4 (D = 64) or all 8 (D = 36): no count asserted)
        assert total(w1, "norm_cert_tiles") > 0 and total(w1, "brackets") < total(w1, "wave_tiles")
        assert nset[0] > 0                                      # (the second sweep may run without the lean launch: the library switches it off when it hands on > 30 % of its tiles)
    if sd == SD_EDGE and K > 2:
        assert total(w1, "brackets") > 0 and all(s < P["n"] for s in nset)
    assert sum(nset) <= 64 * total(w1, "norm_cert_tiles")
    check_sound(P, P["X"], settled)
    check_sn2(sn, sn2, P["R"][0::3])


@pytest.mark.parametrize("D", [64, 36])
@pytest.mark.parametrize("K", [2, 32, 65, "PB_MAXK"])
def test_close_means_take_the_bracket_as_before(pkg, D, K):
    """Means 0.4 sd apart: nothing is settled by the certificate, the brackets are those of option 0, same labels and sub-labels."""
    K = pb_maxk() if K == "PB_MAXK" else K
    P = problem(D, K, SD_CLOSE)
    l1, w1, _, _, settled = run(pkg, P, 2)
    l0, w0, _, _, _ = run(pkg, P, 0)
    assert same(l1, l0)
    assert total(w1, "norm_cert_tiles") == 0 and total(w1, "brackets") == total(w0, "brackets")
    assert not any(f.any() for _, f in settled)


def test_non_finite_features_are_not_settled_by_the_certificate(pkg):
    """A NaN and an Inf feature in two points of different tiles: neither point is in a settled tile, the settled points are a subset of those of
    the clean data less exactly two tiles (2 .. 128 points) in the first sweep, labels and sub-labels are those of option 0."""
    P = problem(64, 32, SD_FAR)
    _, wc, _, _, clean = run(pkg, P, 2)
    c1 = clean[0][1]
    first = int(np.nonzero(c1)[0][0])                           # two points of settled tiles of different clusters
    bad = (first, int(np.nonzero(c1 & (P["z"] != P["z"][first]))[0][0]))
    X = P["X"].copy()
    X[bad[0], 7] = np.nan
    X[bad[1], 60] = np.inf
    l1, w1, _, _, settled = run(pkg, P, 2, X)
    l0, _, _, _, _ = run(pkg, P, 0, X)
    assert same(l1, l0)
    for _, f in settled:
        assert not f[bad[0]] and not f[bad[1]]
    f1 = settled[0][1]
    assert not np.any(f1 & ~c1)
    assert 2 <= int(c1.sum()) - int(f1.sum()) <= 128
    ok = np.ones(P["n"], bool); ok[list(bad)] = False
    check_sound(P, np.where(np.isfinite(X), X, 0.0), [(b, f & ok) for b, f in settled])


def test_automatic_mode_keeps_the_loose_bound_on_a_small_problem(pkg):
    """Option 1 (the default) writes the tight sn2 only where the sweep can earn its cost back: never below 2^22 points.  Here sn2 = sn bit for bit,
    the certificate still runs with it (and settles no more tiles than with the tight bound), labels and sub-labels are those of options 0 and 2."""
    P = problem(64, 32, SD_FAR)
    l1, w1, sn, sn2, settled = run(pkg, P, 1)
    l2, w2, _, _, _ = run(pkg, P, 2)
    l0, _, _, _, _ = run(pkg, P, 0)
    assert np.array_equal(sn2, sn)
    assert same(l1, l0) and same(l1, l2)
    assert total(w1, "norm_cert_tiles") <= total(w2, "norm_cert_tiles")
    check_sound(P, P["X"], settled)


def _device_master_sampler(pkg, X, y, Kt, seed, cert):
    from dpmmsubclusters_jl_amd import binding
    host = importlib.import_module("dpmmsubclusters_jl_amd.host")
    engine = importlib.import_module("dpmmsubclusters_jl_amd.host.engine")
    N, D = X.shape
    prior = host.niw_hyperparams(1.0, np.zeros(D), D + 3, np.eye(D))
    wk = pkg.Worker(pkg.PRIOR_NIW, D, N, device=0, seed=seed)
    wk.upload_points(X)
    wk.set_option(binding.OPT_LEAN_NORM_CERT, cert)
    s = host.DPMMSampler(wk, prior, 10.0, N, seed, burnout=5)
    s._configure()
    s.model.set_option(engine.OPT_DEVICE_MASTER, 1)
    s.start_from_labels(y, 1 + (np.arange(N) & 1), Kt)
    return wk, s


def test_sn2_of_the_device_master(pkg):
    """The table's sn2 block as the device master's hand-over launch writes it, against the Float64 norm of the Float32 factors of the same draw."""
    host = importlib.import_module("dpmmsubclusters_jl_amd.host")
    D, N, Kt = 64, 20000, 6
    X, y = host.gaussian_mixture_shard(N, D, Kt, 100.0, 12345, 0, N)
    wk, s = _device_master_sampler(pkg, X, y, Kt, 11, 2)
    for _ in range(8):
        s.group_step(True, False)
    assert s.K == Kt
    _, sn = wk.debug_pair_ball()
    sn2 = wk.debug_pair_ball_sn2()
    R = np.asarray(s.params["R"], np.float64).reshape(Kt, 3, D, D)[:, 0]
    check_sn2(sn, sn2, R.astype(np.float32))
    wk.close()


def test_same_chain_with_and_without_the_certificate(pkg):
    """A short device-master fit (n = 20 000, D = 64, 8 components, 30 steps, fixed seed) with the option at 0, 1 and 2: equal labels, sub-labels, K
    and parameters at every step -- and the certificate did settle tiles on the way."""
    host = importlib.import_module("dpmmsubclusters_jl_amd.host")
    D, N, Kt = 64, 20000, 8
    X, y = host.gaussian_mixture_shard(N, D, Kt, 100.0, 12345, 0, N)
    hist = {}
    for cert in (0, 1, 2):
        wk, s = _device_master_sampler(pkg, X, y, Kt, 23, cert)
        wk.last_sweep_work()
        steps = []
        for _ in range(30):
            s.group_step(False, False)
            lab, sub = wk.get_labels()
            p = s.params
            steps.append((s.K, lab, sub, np.array(p["mu"]), np.array(p["R"]), np.array(p["logdet"])))
        hist[cert] = (steps, total(wk.last_sweep_work(), "norm_cert_tiles"))
        wk.close()
    assert hist[0][1] == 0 and hist[2][1] > 0
    for other in (1, 2):
        for a, b in zip(hist[0][0], hist[other][0]):
            assert a[0] == b[0]
            for u, v in zip(a[1:], b[1:]):
                assert np.array_equal(u, v)
