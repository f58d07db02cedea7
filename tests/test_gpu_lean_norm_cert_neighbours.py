"""The norm certificate with the tight norm sn2 for EVERY cluster (DPMM_OPT_LEAN_NORM_CERT, csrc/niw_lean.hip, csrc/niw_b3.h): the certificate's pair-ball
loop in niw_lean_kernel bounds the neighbours' |R_j (x - mu_k0)| with sn2_j where the table's block is tight; option 3 keeps sn for them (the earlier
behaviour, for comparisons).  Checked here: the table's sn2 from both of its producers against the same power bound in Float64 numpy; labels and
sub-labels bit-identical for the option at 0, 1, 2 and 3; every point of a settled tile cleared by a Float64 evaluation; 2 settles no fewer tiles than 3."""
import importlib

import numpy as np
import pytest

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

MARGIN = 50.0        # the library's default screen margin
M_SQUARINGS = 3      # PB_NORM_SQUARINGS (csrc/dpmm_kernels.h)
TABLE_D = [33, 36, 48, 64]     # 36, 48: padded rows.  33: the library keeps NO pair-ball table where D is not a multiple of 4 (the table lives with the tail
                               # records, dpmm_api.cpp have_tail) -- the case stays and checks that the library says so instead of handing out a stale block


def no_table(wk):
    from dpmmsubclusters_jl_amd import binding
    with pytest.raises(binding.DpmmError, match="no pair-ball table"):
        wk.debug_pair_ball()
    with pytest.raises(binding.DpmmError, match="no pair-ball table"):
        wk.debug_pair_ball_sn2()


@pytest.fixture(scope="module")
def pkg():
    return load_package()


# ------------------------------------------------------------------------------------------------------------------ the table
def power_bound(R32, sn):
    """pair_ball_block's sn2 for one Float32 factor, in Float64: P = R' R, M squarings each behind a power-of-two rescaling to a largest row sum in
    [1/2, 1), the last row sum, the roots, the factors 1 + 1e-6 (on s^2) and 1 + 1e-7, rounded to Float32, clamped to sn."""
    R = R32.astype(np.float64)
    p = R.T @ R
    cs = []
    t = 0.0
    for step in range(M_SQUARINGS + 1):
        t = np.abs(p).sum(axis=1).max()
        if step == M_SQUARINGS:
            break
        ex = int(np.frexp(t)[1]) if (t > 0 and np.isfinite(t)) else 0
        cs.append(np.ldexp(1.0, ex))
        p = p * np.ldexp(1.0, -ex)
        p = p @ p
    bound = np.sqrt(t)
    for step in range(M_SQUARINGS - 1, 0, -1):
        bound = np.sqrt(cs[step] * bound)
    bound *= cs[0]
    with np.errstate(over="ignore"):
        s2 = np.float32(np.sqrt(bound * (1.0 + 1e-6)) * (1.0 + 1e-7))
    return s2 if (s2 == s2 and s2 < sn) else sn


def factors(kind, D, K, rng):
    """K upper-triangular Float32 factors R (R' R = a precision).  'wishart': Q diag(lambda) Q' with lambda spread over 1e4; 'rows': a Wishart factor
    whose rows are scaled by 10^(-2 .. 2) in a shuffled order (a permuted or transposed block of R' R changes the norm); 'diag': diagonal."""
    out = np.zeros((K, D, D), np.float32)
    for k in range(K):
        if kind == "diag":
            out[k] = np.diag(10.0 ** rng.uniform(-2, 2, D))
            continue
        if kind == "wishart":
            Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
            lam = 10.0 ** rng.uniform(-2, 2, D)
            lam[0], lam[1] = 1e-2, 1e2                           # (the spread is there whatever the draw)
            C = np.linalg.cholesky((Q * lam) @ Q.T)
            out[k] = C.T
        else:
            G = rng.normal(size=(D, D + 2))
            C = np.linalg.cholesky(G @ G.T)
            out[k] = rng.permutation(10.0 ** np.linspace(-2, 2, D))[:, None] * C.T
    return out


def table_of(pkg, D, Rk, cert=2):
    """sn, sn2 as launch_niw_b3_pack writes them for the cluster-level factors Rk (K, D, D)."""
    from dpmmsubclusters_jl_amd import binding
    K = len(Rk)
    n = 64
    rng = np.random.default_rng(5)
    wk = pkg.Worker(pkg.PRIOR_NIW, D, n, first_index=0, device=0, seed=3)
    wk.upload_points(rng.normal(size=(n, D)).astype(np.float32))
    wk.set_option(binding.OPT_LEAN_NORM_CERT, cert)
    if K > 64:
        wk.set_option(binding.OPT_PRESCREEN, 0)
    mu = rng.normal(size=(3 * K, D)).astype(np.float32)
    R = np.repeat(Rk, 3, axis=0)
    with np.errstate(all="ignore"):
        logdet = np.zeros(3 * K, np.float32)
    wk.set_params_niw_chol(mu, R, logdet, np.full((K, 2), 0.5, np.float32), np.full(K, 1.0 / K, np.float32))
    if D % 4:
        no_table(wk)
        wk.close()
        return None, None
    _, sn = wk.debug_pair_ball()
    sn2 = wk.debug_pair_ball_sn2()
    wk.close()
    return sn, sn2


def check_table(sn, sn2, Rk, what):
    true_s = np.linalg.norm(Rk.astype(np.float64), 2, axis=(1, 2))
    want = np.array([power_bound(Rk[k], sn[k]) for k in range(len(Rk))], np.float32)
    rel = np.abs(sn2.astype(np.float64) - want) / want
    print(f"   {what}: sn2 / |R|_2 {np.min(sn2 / true_s):.6f} .. {np.max(sn2 / true_s):.4f}; sn / |R|_2 max {np.max(sn / true_s):.4f}; "
          f"|sn2 - numpy| / numpy max {rel.max():.2e}; clamped {int((sn2 == sn).sum())} of {len(sn)}")
    assert np.all(sn2 > true_s)
    assert np.all(sn2 <= sn)
    assert np.all(rel <= 1e-6)


@pytest.mark.parametrize("D", TABLE_D)
@pytest.mark.parametrize("K", [2, 3, 33, 64, 65, 256])
def test_table_of_the_pack_kernel(pkg, D, K):
    """launch_niw_b3_pack, option 2: sn2 > |R|_2 (Float64 numpy on the Float32 factors), sn2 <= sn, and sn2 = numpy's same power bound to 1e-6 -- for
    factors with a spectrum spread of 1e4, with strongly unequal row scales, and diagonal ones."""
    rng = np.random.default_rng(100 * D + K)
    for kind in ("wishart", "rows", "diag"):
        Rk = factors(kind, D, K, rng)
        sn, sn2 = table_of(pkg, D, Rk)
        if sn is not None:
            check_table(sn, sn2, Rk, f"D={D} K={K} {kind}")


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


@pytest.mark.parametrize("D", TABLE_D)
@pytest.mark.parametrize("K", [2, 3, 33, 64, 65, 256])
def test_table_of_the_device_master(pkg, D, K):
    """The hand-over launch's role, option 2, on the factors the device master drew: components far apart, feature scales 10^(-1 .. 1) in a shuffled
    order (covariances with a spectrum spread of 1e4 and unequal rows in the factor); the same three checks on the Float32 factors of that draw."""
    rng = np.random.default_rng(7 * D + K)
    per = 40
    N = per * K
    y = np.repeat(np.arange(1, K + 1), per)
    scale = rng.permutation(10.0 ** np.linspace(-1, 1, D))
    X = ((rng.normal(size=(K, D)) * 300.0)[y - 1] + rng.normal(size=(N, D)) * scale).astype(np.float32)
    wk, s = _device_master_sampler(pkg, X, y, K, 11, 2)
    for _ in range(2):
        s.group_step(True, False)
    assert s.K == K
    if D % 4:
        no_table(wk)
        wk.close()
        return
    _, sn = wk.debug_pair_ball()
    sn2 = wk.debug_pair_ball_sn2()
    Rk = np.asarray(s.params["R"], np.float64).reshape(K, 3, D, D)[:, 0].astype(np.float32)
    wk.close()
    if not np.any(np.triu(Rk, 1)):                             # (stored column by column: read row by row it is the transpose -- R is the UPPER factor)
        Rk = np.ascontiguousarray(Rk.transpose(0, 2, 1))
    check_table(sn, sn2, Rk, f"device master D={D} K={K}")


@pytest.mark.parametrize("D", [36, 64])
def test_table_edge_cases(pkg, D):
    """Factors scaled by 2^60 and by 2^-60 stay certified or fall back to sn; a NaN in R leaves sn2 = sn = inf for that cluster and the others as they are."""
    rng = np.random.default_rng(D)
    K = 5
    base = factors("rows", D, K, rng)
    for sc in (2.0 ** 60, 2.0 ** -60):
        Rk = (base.astype(np.float64) * sc).astype(np.float32)
        Rk[1:] = base[1:]                                        # (one scaled cluster among ordinary ones)
        sn, sn2 = table_of(pkg, D, Rk)
        true_s = np.linalg.norm(Rk.astype(np.float64), 2, axis=(1, 2))
        print(f"   D={D} scale {sc:.3g}: sn {sn[0]:.6g} sn2 {sn2[0]:.6g} |R|_2 {true_s[0]:.6g}")
        assert np.all(sn2 <= sn)
        assert sn2[0] > true_s[0] or sn2[0] == sn[0]
        check_table(sn[1:], sn2[1:], Rk[1:], "the other clusters")
    Rk = base.copy()
    Rk[2, 3, D - 2] = np.nan
    sn, sn2 = table_of(pkg, D, Rk)
    assert np.isinf(sn[2]) and sn[2] > 0 and np.isinf(sn2[2]) and sn2[2] > 0
    ok = np.arange(K) != 2
    check_table(sn[ok], sn2[ok], Rk[ok], "the clusters without a NaN")


# ------------------------------------------------------------------------------------------------------------------ sweeps
_PROBLEMS = {}


def problem(D, K, sd, n):
    """K components with covariances InvWishart(D + 2, I) (as the bench generator draws them), means N(0, sd^2 I), n points in component order;
    the sub-clusters share the component's covariance, their means sit a little apart.  The Float32 parameters are the ones the worker is given."""
    key = (D, K, sd, n)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    rng = np.random.default_rng(1000 * D + 10 * K + int(10 * sd) + 7 * n)
    mu = np.zeros((3 * K, D), np.float32); R = np.zeros((3 * K, D, D), np.float32); logdet = np.zeros(3 * K, np.float32)
    z = np.minimum(np.arange(n) * K // n, K - 1)
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
    D, K = P["D"], P["K"]
    mu = P["mu"][0::3].astype(np.float64); R = P["R"][0::3].astype(np.float64)
    cst = -0.5 * P["logdet"][0::3].astype(np.float64) + np.log(P["w"].astype(np.float64))
    X = X.astype(np.float64)
    a = np.empty((len(X), K))
    for j in range(K):
        y = (X - mu[j]) @ R[j].T
        a[:, j] = cst[j] - 0.5 * (y * y).sum(1)
    return a


def total(w, k):
    return round(w[k] * max(1, w["launches"]))                  # (the counters come back per launch)


def run(pkg, P, cert, sweeps, X=None):
    """`sweeps` sweeps of a chain from fixed parameters (each on the labels of the one before).  Returns the labels and sub-labels after each, the work
    counters of all of them and, per sweep, (labels before the sweep, flags of the points whose tile the certificate settled)."""
    from dpmmsubclusters_jl_amd import binding
    D, K, n = P["D"], P["K"], P["n"]
    wk = pkg.Worker(pkg.PRIOR_NIW, D, n, first_index=0, device=0, seed=41)
    wk.upload_points(P["X"] if X is None else X)
    wk.set_option(binding.OPT_LEAN_NORM_CERT, cert)
    if K > 64:
        wk.set_option(binding.OPT_PRESCREEN, 0)
    par = (P["mu"], P["R"], P["logdet"], P["lr"], P["w"])
    wk.set_params_niw_chol(*par)
    wk.set_labels(P["z"] + 1, 1 + (np.arange(n) & 1))
    wk.suffstats_packed(None)                                  # the bin-sorted visiting order
    wk.set_params_niw_chol(*par)
    wk.last_sweep_work()
    wk.debug_norm_cert_points(enable=True, read=False)
    labs, settled = [], []
    before = P["z"] + 1
    for ep in range(1, sweeps + 1):
        wk.sweep(ep)
        labs.append(wk.get_labels())
        settled.append((before, wk.debug_norm_cert_points(enable=True)))
        before = labs[-1][0]
        wk.suffstats_packed(None)
        wk.set_params_niw_chol(*par)
    work = wk.last_sweep_work()
    wk.close()
    return labs, work, settled


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


@pytest.mark.parametrize("n", [1, 63, 64, 64 * 3 + 17, 5000])
@pytest.mark.parametrize("K", [2, 5, 33, 65])
def test_same_labels_whatever_the_option(pkg, n, K):
    """Six sweeps of a chain with the option at 0, 1, 2 and 3: equal labels and sub-labels after every sweep, for component means 30, 6 and 2 standard
    deviations apart (everything settled, a mix, nothing settled) and one point with a NaN feature (n >= 63).  At 6 sd with n = 5000 and K >= 5 the
    certificate settles some tiles and leaves others."""
    for sd in (30.0, 6.0, 2.0):
        P = problem(64, K, sd, n)
        X = P["X"].copy()
        if n >= 63:
            X[n // 2, 11] = np.nan
        res = {cert: run(pkg, P, cert, 6, X) for cert in (0, 1, 2, 3)}
        tiles = {c: total(res[c][1], "norm_cert_tiles") for c in res}
        print(f"n={n} K={K} sd={sd}: tiles {total(res[2][1], 'wave_tiles')}, settled by the certificate {tiles}, brackets {total(res[2][1], 'brackets')}")
        for cert in (1, 2, 3):
            assert same(res[cert][0], res[0][0]), (sd, cert)
        assert tiles[0] == 0
        assert tiles[2] >= tiles[3]
        if sd == 6.0 and n == 5000 and K >= 5:
            assert tiles[2] > 0 and total(res[2][1], "brackets") > 6      # (more than the NaN point's tile of every sweep)
        if n >= 63:
            for _, f in res[2][2]:
                assert not f[n // 2]                            # (the NaN point's tile is never settled by the certificate)


@pytest.mark.parametrize("D", [64, 36])
@pytest.mark.parametrize("K", [5, 33, 65])
def test_settled_points_are_cleared_in_float64(pkg, D, K):
    """Means 6 sd apart, option 2: for every point of a tile the certificate settled, a_j(x) < a_k0(x) - margin for all j != k0 in Float64; and the
    certificate settles at least as many tiles as under option 3 (the neighbours bounded with sn) on the same parameters."""
    P = problem(D, K, 6.0, 64 * 3 * K + 17)
    l2, w2, settled = run(pkg, P, 2, 2)
    l3, w3, settled3 = run(pkg, P, 3, 2)
    t2, t3 = total(w2, "norm_cert_tiles"), total(w3, "norm_cert_tiles")
    print(f"D={D} K={K}: tiles {total(w2, 'wave_tiles')}, settled by the certificate: option 2 {t2}, option 3 {t3}")
    assert same(l2, l3)
    assert t2 >= t3
    a = loglik64(P, P["X"])
    for stl in (settled, settled3):
        for before, flags in stl:
            i = np.nonzero(flags)[0]
            k0 = before[i] - 1
            own = a[i, k0]
            rest = a[i].copy()
            rest[np.arange(len(i)), k0] = -np.inf
            assert np.all(rest.max(axis=1) < own - MARGIN)
    assert any(f.any() for _, f in settled)
