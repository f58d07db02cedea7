"""GPU tests of the Student-t predictive table -- the epilogue `a = cst[3k] - hdf log1pf(q / df)` of niw_sweep_kernel and
niw_sweep_direct_kernel (NB = 1, 2, 4, 8, 16), dpmm_set_predictive_niw's constant, host/priors.py's conversion of a posterior -- and of the
numbers users get from it (score_samples, predict) against a Float64 closed form.  It is the independent anchor of the table that
tests/test_gpu_score.py takes as its reference.

The reference (tests/tools/predictive_ref.py, checked on the CPU by tests/test_predictive_reference_cpu.py against scipy's multivariate t):
    want[k, i] = lgamma((df+D)/2) - lgamma(df/2) - D/2 log(df pi) - logdet/2 + log w - (df+D)/2 log1p(q / df),   q = |R_k (x_i - m_k)|^2
in Float64 on the Float32 parameters and points the library receives; for posteriors, scipy's multivariate t of the posterior itself
(oracle.niw_posterior_predictive) + log w.

The bound, per entry, from the Float64 evaluation alone (u = 2^-24):
    e_i = (D + 2) u sum_j |R_ij| |z_j|                    y = R z: the subtraction z = x - m, D products, D - 1 Float32 additions in any order
    dq = 2 sum_i |y_i| e_i + sum_i e_i^2 + (D + 1) u q    q = sum y_i^2: the error of y carried through the squares, the squares, their sum
    bound = hdf dq / (df + q)                             |da/dq| dq
          + 2^-21 (|cst| + hdf log1p(q / df))             Float32 cst, the division, a few-ulp log1pf, the product, the subtraction
          + 1e-6
    posteriors: e_i has (D + 3): the Float32 rounding of the converted R, u sum_j |R_ij| |z_j| per row.
    log-density: max over the clusters of the bounds at the point + 2^-23 (K + 16), the finish kernel's term of tests/test_gpu_score.py.
The kernel's q overflows to +Inf where the Float64 q is beyond FLT_MAX (the planted 1e25 point: q about 1e50 D): the entry is -Inf while
the reference is finite; asserted exactly there, and the planted magnitudes are far from that threshold on both sides.

Measured on an MI355X, max |got - want| / bound per case (printed by every test):
    table, K = 3:   D=1 0.162   D=2 0.153   D=5 0.156   D=16 0.138   D=17 0.145   D=32 0.063   D=33 0.075   D=48 0.069   D=63 0.070
                    D=64 0.048   D=65 0.102   D=100 0.051   D=128 0.026   D=129 0.095   D=200 0.070   D=256 0.076
    table, other K: D=2 K=1 0.147   D=64 K=1 0.057   D=8 K=45 0.158   D=24 K=60 0.144   D=64 K=90 0.112   D=128 K=70 0.059
                    (the maxima sit at entries of small q, where the bound is little more than the rounding of cst; at the points
                    1e3 sd out the ratio is at most 0.14)
    after a sweep:  D=64 0.032   D=128 0.017
    posteriors:     D=2 0.186   D=20 0.289   D=64 0.056   D=70 0.145   D=256 0.079
    fitted model (K = 4): score_samples 0.057 of its tolerance (both entry points); predict 0.041 of 2 max bound over 600 points
"""
import importlib

import numpy as np
import pytest

from oracle import oracle as orc
from tools import predictive_ref as pr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def host(pkg):
    return importlib.import_module(pkg.__name__ + ".host")


@pytest.fixture(scope="module")
def priors(pkg):
    return importlib.import_module(pkg.__name__ + ".host.priors")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def params_of(c):
    return c["m"], c["R"].reshape(c["K"], -1), c["logdet"], c["df"], c["w"]


def reference_of(c, X=None):
    X = c["X"] if X is None else X
    want, parts = pr.student_t_table(X, c["m"], c["R"], c["logdet"], c["df"], c["w"])
    return want, parts, pr.error_bound(X, c["m"], c["R"], c["df"], parts)


# ------------------------------------------------------------------------------------------------ the table against the reference
@pytest.mark.parametrize("D,K", pr.CASES)
def test_table_against_float64_closed_form(pkg, D, K):
    c = pr.make_case(D, K)
    want, parts, bound = reference_of(c)
    wk = pkg.Worker(pkg.PRIOR_NIW, D, c["n"], device=0, seed=1)
    try:
        wk.upload_points(c["X"])
        got = wk.predict_table_niw(*params_of(c))
    finally:
        wk.close()
    assert got.shape == (K, c["n"]) and got.dtype == np.float32
    # planted points first (they say more than a ratio): the mean (q = 0: the constant, bit for bit), 1e25 (-Inf), NaN
    for i, k in c["planted"]["mean"]:
        assert bits(got[k, i]) == bits(np.float32(parts["cst"][k])), (k, got[k, i], parts["cst"][k])
    for i in c["planted"]["huge"]:
        assert np.all(np.isneginf(got[:, i])), got[:, i]
    for i, _ in c["planted"]["nan"]:
        assert np.isnan(got[:, i]).all(), got[:, i]
    worst = pr.check_table(got, want, bound, parts["q"])
    far = max(float(abs(got[k, i] - want[k, i]) / bound[k, i]) for i, k in c["planted"]["far"])
    print(f"D={D} K={K}: max |got - want| / bound = {worst:.3f} (1e3 sd points: {far:.3f})")
    # second anchor: a cluster of df = 1e6 is the Gaussian -D/2 log(2 pi) - logdet/2 - q/2 + log w within (q^2 + D^2) / df
    big = np.flatnonzero(c["df"] == np.float32(1e6))
    assert (len(big) > 0) == (K >= 3)
    if len(big):
        gauss = pr.gaussian_table(parts, c["logdet"], c["w"], D)[big]
        fin = np.isfinite(got[big])
        slack = bound[big] + (parts["q"][big] ** 2 + D * D) / 1e6
        d = np.abs(got[big].astype(np.float64) - gauss)
        assert np.all(d[fin] <= slack[fin]), float((d[fin] / slack[fin]).max())
        assert np.median(slack[:, c["bulk"]]) < 0.2 * max(D, 4)               # (the anchor says something on the bulk)


@pytest.mark.parametrize("D", [64, 128])
def test_table_mode_after_sweep_mode_and_back(pkg, D):
    """One worker: sweep parameters and a sweep, predictive parameters, sweep parameters again.  The table is what a fresh worker
    computes (A.tdf doubles as a tile list in other instantiations; the `predictive` flag of dpmm_api.cpp), and the sweep behind it
    again equals the oracle's draw on the worker's own Gaussian table."""
    K, seed, first = 3, 123456789, 1000003
    c = pr.make_case(D, K)
    X = c["X"].copy()
    X[~c["bulk"]] = X[c["bulk"]][:7]                                       # a sweep draws labels: finite points only
    want, parts, bound = reference_of(c, X)
    n = c["n"]
    rng = np.random.default_rng(D)
    mus = np.repeat(c["m"].astype(np.float64), 3, axis=0)
    mus[1::3] += 0.3
    mus[2::3] -= 0.3
    A = rng.normal(size=(3 * K, D, D)) * (0.3 / np.sqrt(D))
    Sig = A @ A.transpose(0, 2, 1) + np.eye(D)
    invS = np.linalg.inv(Sig)
    invS = 0.5 * (invS + invS.transpose(0, 2, 1))
    sweep_params = (mus, invS.reshape(3 * K, -1), np.linalg.slogdet(Sig)[1], np.full((K, 2), 0.5, np.float32), c["w"])

    fresh = pkg.Worker(pkg.PRIOR_NIW, D, n, first_index=first, device=0, seed=seed)
    wk = pkg.Worker(pkg.PRIOR_NIW, D, n, first_index=first, device=0, seed=seed)
    try:
        fresh.upload_points(X)
        tab_fresh = fresh.predict_table_niw(*params_of(c))
        wk.upload_points(X)
        wk.set_params_niw(*sweep_params)
        wk.sweep(1)
        tab = wk.predict_table_niw(*params_of(c))
        assert np.array_equal(bits(tab), bits(tab_fresh))
        print(f"D={D}: after a sweep, max |got - want| / bound = {pr.check_table(tab, want, bound, parts['q']):.3f}")
        with pytest.raises(pkg.DpmmError):                                 # predictive parameters are no sweep parameters
            wk.sweep(2)
        wk.set_params_niw(*sweep_params)
        wk.sweep(2)
        lab, sub = wk.get_labels()
        gtab = wk.debug_loglik()
        u0, u1 = orc.uniforms(seed, 2, 0, first, n)
        assert np.array_equal(orc.sample_log_cat(gtab, u0), lab)
        tab2 = wk.debug_subloglik()
        i = np.arange(n)
        assert np.array_equal(orc.sample_log_cat(np.stack([tab2[2 * (lab - 1), i], tab2[2 * (lab - 1) + 1, i]]), u1), sub)
        # and the Gaussian table is the sweep parameters' (Float64, the tolerance of test_loglik_table), not a Student-t one
        g64 = np.stack([orc.niw_loglik_f64(X, D, np.float32(mus[3 * k]), np.float32(invS[3 * k]).ravel(), np.float32(sweep_params[2][3 * k]))
                        + np.log(np.float64(c["w"][k])) for k in range(K)]) + 0.5 * D * D * np.log(2 * np.pi)
        assert np.all(np.abs(gtab - g64) <= 1e-3 + 2e-5 * np.abs(g64))
        assert np.array_equal(bits(wk.predict_table_niw(*params_of(c))), bits(tab_fresh))      # and once more
    finally:
        fresh.close()
        wk.close()


# ------------------------------------------------------------------------------------------------ the host conversion
@pytest.mark.parametrize("D", pr.POSTERIOR_DIMS)
def test_conversion_of_hand_made_posteriors(pkg, priors, D):
    P = pr.make_posterior(D)
    prior = priors.niw_hyperparams(1.0, np.zeros(D), D + 3.0, np.eye(D))
    rows = list(range(P["K"]))
    cap = pr.Capture()
    prior.predictive_table(cap, P["post"], rows, P["w"])
    want, parts, bound = pr.posterior_reference(P, cap.args, orc.niw_posterior_predictive)
    wk = pkg.Worker(pkg.PRIOR_NIW, D, P["n"], device=0, seed=1)
    try:
        wk.upload_points(P["X"])
        got = prior.predictive_table(wk, P["post"], rows, P["w"])
    finally:
        wk.close()
    print(f"D={D}: posterior -> table, max |got - want| / bound = {pr.check_table(got, want, bound, parts['q']):.3f}")


# ------------------------------------------------------------------------------------------------ the user-facing numbers
@pytest.fixture(scope="module")
def fitted(host):
    """The fit of tests/test_gpu_score.py (3000 points, D = 8, 25 iterations), query points between the cluster means, and the Float64
    reference: scipy's component log-densities + log w, w = (points_count + alpha) / sum as host/api.py forms it (a Float32).  The
    components are evaluated at the Float32 rounding of the posterior means -- the library's interface is Float32; m passes through the
    conversion unchanged."""
    x, _, _, _ = host.generate_gaussian_data(3000, 8, 4, 20.0, seed=5)
    model = host.fit(x, 10.0, iters=25, seed=11, burnout=5, verbose=False)[-1]
    s = model.sampler
    K, D = s.K, 8
    rows = [3 * k for k in range(K)]
    post = {key: np.asarray(s.post[key])[rows] for key in ("kappa", "nu", "m", "U")}
    w = s.points_count.astype(np.float64) + s.alpha
    w = (w / w.sum()).astype(np.float32)
    post32 = dict(post, m=post["m"].astype(np.float32).astype(np.float64))
    cap = pr.Capture()
    s.prior.predictive_table(cap, post, list(range(K)), w)
    # query points: candidates on the segments between two cluster means, 600 of those where the reference's two best clusters are
    # within 10 nats of each other (they decide whether the probabilities say anything) and 600 of the others
    rng = np.random.default_rng(21)
    nc = 12000
    a = rng.integers(0, K, nc)
    b = (a + rng.integers(1, K, nc)) % K
    t = rng.uniform(0.25, 0.75, nc)[:, None]
    cand = (post["m"][a] * (1 - t) + post["m"][b] * t + 0.5 * rng.standard_normal((nc, D))).astype(np.float32)
    top2 = -np.sort(-pr.posterior_reference(dict(X=cand, post=post32, w=w, K=K), cap.args, orc.niw_posterior_predictive)[0], axis=0)[:2]
    near = top2[0] - top2[1] < 10.0
    X = np.concatenate([cand[near][:600], cand[~near][:600]])
    P = dict(X=X, post=post32, w=w, K=K)
    comp, parts, bound = pr.posterior_reference(P, cap.args, orc.niw_posterior_predictive)       # (K, n): log-density + log w
    M = comp.max(0)
    logdens = M + np.log(np.exp(comp - M).sum(0))
    return dict(model=model, X=X, K=K, comp=comp, logdens=logdens, bound=bound.max(0))


def test_score_samples_is_the_log_of_the_mixture_density(host, fitted):
    f = fitted
    assert f["K"] >= 2
    tol = f["bound"] + EPS * (f["K"] + 16)
    data = np.ascontiguousarray(f["X"].T)
    with host.Predictor(f["model"], capacity=517) as p:
        got_p = np.asarray(p.score_samples(data))
    got_h = np.asarray(host.score_samples(f["model"], data))
    for name, got in (("Predictor.score_samples", got_p), ("host.score_samples", got_h)):
        assert got.shape == f["logdens"].shape and got.dtype == np.float32
        d = np.abs(got.astype(np.float64) - f["logdens"])
        print(f"{name}: K={f['K']}, max |got - want| / tolerance = {float((d / tol).max()):.3f} (largest tolerance {tol.max():.2e})")
        assert np.all(d <= tol)


def test_predict_probabilities_where_two_clusters_compete(host, fitted):
    f = fitted
    order = np.argsort(-f["comp"], axis=0)
    best, second = order[0], order[1]
    i = np.arange(f["comp"].shape[1])
    close = np.flatnonzero(f["comp"][best, i] - f["comp"][second, i] < 10.0)
    assert len(close) >= 200, len(close)                                   # not saturated: from the reference alone
    labels, probs = host.predict(f["model"], np.ascontiguousarray(f["X"].T))
    probs = np.asarray(probs, np.float64)
    want_log = f["comp"] - f["logdens"][None, :]
    tol = 2 * f["bound"][close]
    worst = 0.0
    for which in (best, second):
        d = np.abs(np.log(probs[close, which[close]]) - want_log[which[close], close])
        worst = max(worst, float((d / tol).max()))
        assert np.all(d <= tol)
    print(f"predict: {len(close)} points with two clusters within 10 nats, max |log p - want| / (2 max bound) = {worst:.3f}")
    clear = f["comp"][best, i] - f["comp"][second, i] > 4 * f["bound"]
    assert np.array_equal(np.asarray(labels)[clear], best[clear] + 1)
