"""GPU tests of the conditional CDF and quantiles of the targets (include/dpmm_hip_regress_cdf.h, csrc/regress_cdf.hip) through host/score.py's
Regressor.cdf / quantile / interval and the one-shots.

The reference is tests/tools/regress_cdf_ref.py (Float64, scipy's Student-t, from the GPU's own p_ik; checked on the CPU by
tests/test_regress_cdf_cpu.py): every cdf and sf entry must lie within the header's b_F, every quantile within the probability-space
contract |F_exact(y) - level| <= b_F + f_exact (y - y-), b_F and f_exact the larger of their values at y and at its Float32 predecessor y-.
Shapes: regress_cdf_ref.SHAPES x KS, n over NS, overlapping and separated models.
"""
import functools
import importlib

import numpy as np
import pytest

from tools import predictive_ref as pr
from tools import regress_cdf_ref as rc
from tools import regress_ref as rr

pytestmark = pytest.mark.gpu

CAP = 64
# (D_o, D_t, K, n, overlapping): every shape with every K, every n with every shape or K; the wide cases at K = 40 with few points (the
# Float64 reference is n K D_t Student-t evaluations, a dozen times)
CASES = [(1, 1, 1, 1, True), (1, 1, 3, 33, True), (1, 1, 40, 229, True), (5, 31, 1, 31, True), (5, 31, 3, 229, False), (5, 31, 40, 31, True),
         (32, 33, 1, 33, False), (32, 33, 3, 1, True), (32, 33, 40, 33, True), (33, 130, 1, 229, True), (33, 130, 3, 31, True), (33, 130, 40, 33, False),
         (7, 249, 1, 1, True), (7, 249, 3, 33, False), (7, 249, 40, 1, False), (5, 31, 3, 1, True)]
assert {c[:2] for c in CASES} == set(rc.SHAPES) and {c[2] for c in CASES} == set(rc.KS) and {c[3] for c in CASES} == set(rc.NS)


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


@functools.lru_cache(maxsize=None)
def case(Do, Dt, K, n, overlap=True, low_df=False):
    return rc.make_case(Do, Dt, K, n, overlap=overlap, low_df=low_df)


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def to_np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def open_regressor(score, c, capacity=CAP, **kw):
    parent = score.Predictor(rr.dummy_model(c["post"], c["K"], c["D"]), capacity=capacity, **kw)
    return parent, parent.regressor(c["given"], c["targets"])


def held(reg, X):
    """What the reference needs of the worker's state: the tables, q (n, K) of the marginal model and the bound t of its table entries."""
    B, cc, V, hk, df = reg.tables()
    m, R, logdet, dff, w = (np.asarray(a, np.float32) for a in reg.marginal._predictive_args()[1])
    want, parts = pr.student_t_table(X, m, R, logdet, dff, w)
    parts["want"] = want
    t = pr.error_bound(X, m, R, dff, parts).T
    return dict(B=B, c=cc, V=V, df=df, h=hk, q=parts["q"].T, t=t, x=X.astype(np.float64))


def ref_cdf(h, probs, y):
    return rc.cdf(probs, h["B"], h["c"], h["V"], h["df"], h["q"], h["x"], y, t=h["t"])


def worst(got, want, bound):
    fin = np.isfinite(want)
    assert np.isfinite(got[fin]).all()
    return float((np.abs(got[fin].astype(np.float64) - want[fin]) / bound[fin]).max())


@pytest.mark.parametrize("Do,Dt,K,n,overlap", CASES)
def test_cdf_and_quantiles_against_float64(score, Do, Dt, K, n, overlap):
    c = case(Do, Dt, K, n, overlap)
    data, y = np.ascontiguousarray(c["X"].T), np.ascontiguousarray(c["Y"].T)
    parent, reg = open_regressor(score, c)
    with parent, reg:
        res = reg.cdf(data, y.astype(np.float64))                        # (any real dtype)
        mean = reg.predict(data)
        # 40 sigma out on either side of the mixture's mean: one of cdf / sf must keep its relative accuracy
        spread = 40.0 * float(np.max(c["s"]))
        far = np.where(np.arange(n)[None, :] % 2 == 0, mean.mean + spread, mean.mean - spread).astype(np.float32)
        out = reg.cdf(data, far)
        qs = reg.quantile(data, rc.LEVELS)
        back = [reg.cdf(data, qs.values[j]) for j in range(len(rc.LEVELS))]
        lab, probs = reg.marginal.predict(data)
        entry = reg.marginal.score_samples(data)
        h = held(reg, c["X"])
    assert res.cdf.shape == (Dt, n) and res.sf.shape == (Dt, n) and res.cdf.dtype == np.float32 and res.skipped == 0 and qs.skipped == 0
    assert np.array_equal(res.labels, lab) and np.array_equal(qs.labels, lab) and np.array_equal(res.labels, mean.labels)
    ref = ref_cdf(h, probs, c["Y"])
    r_c, r_s = worst(res.cdf.T, ref["cdf"], ref["b_cdf"]), worst(res.sf.T, ref["sf"], ref["b_sf"])
    ref = ref_cdf(h, probs, far.T)
    r_fc, r_fs = worst(out.cdf.T, ref["cdf"], ref["b_cdf"]), worst(out.sf.T, ref["sf"], ref["b_sf"])
    small = np.minimum(ref["cdf"], ref["sf"])
    assert small.min() > 0
    normal = small >= 2.0 ** -100                                        # (where Float32 can hold the value: below, the bound is its underflow term)
    if normal.any():                                                     # the bound is RELATIVE out there: the side that does not cancel keeps its digits
        assert np.median((np.minimum(ref["b_cdf"], ref["b_sf"]) / small)[normal]) < 1e-2
    assert np.all(np.minimum(out.cdf, out.sf).T[small >= 2.0 ** -126] > 0)      # (not 0 by cancellation; below Float32's range 0 is the rounding)
    # ---- the quantiles: the contract in probability; monotone; K = 1 closed form
    assert qs.values.shape == (len(rc.LEVELS), Dt, n) and qs.values.dtype == np.float32 and qs.levels == tuple(rc.LEVELS)
    assert np.all(np.diff(qs.values, axis=0) >= 0)
    r_q = r_b = 0.0
    for j, lv in enumerate(rc.LEVELS):
        err, bound = rc.quantile_contract(probs, h["B"], h["c"], h["V"], h["df"], h["q"], h["x"], qs.values[j].T, lv, t=h["t"])
        r_q = max(r_q, float((err / bound).max()))
        # cdf(x, quantile(x, level)) gives the level back: within the contract plus the bound of the cdf call itself; above 1 / 2 it is
        # sf, the side that does not cancel, that gives 1 - level back as accurately
        at = ref_cdf(h, probs, qs.values[j].T)
        r_b = max(r_b, float((np.abs(back[j].cdf.T.astype(np.float64) - lv) / (bound + at["b_cdf"])).max()),
                  float((np.abs(back[j].sf.T.astype(np.float64) - (probs.astype(np.float64).sum(1, keepdims=True) - lv)) / (bound + at["b_sf"])).max()))
    several = float(((probs != 0).sum(1) > 1).mean())
    print(f"Do={Do} Dt={Dt} K={K} n={n} overlap={overlap}: points with several clusters {several:.2f}; worst got / bound: cdf {r_c:.2e} sf {r_s:.2e} "
          f"far cdf {r_fc:.2e} far sf {r_fs:.2e} quantile {r_q:.2e} cdf(quantile) {r_b:.2e}")
    assert max(r_c, r_s, r_fc, r_fs) <= 1.0 and r_q <= 1.0 and r_b <= 1.0
    if K > 1 and overlap and Do <= 7:
        assert several > 0.5
    if K == 1:
        # one cluster: level 1 / 2 is `mean` bit for bit; the others are mu + sigma z within 2 ulp32, sigma from q as the kernel recovers it
        # from its own table entry (K = 1: the entry is the log-density score_samples returns)
        assert np.array_equal(bits(qs.values[2]), bits(mean.mean))
        z = stats_ppf(rc.LEVELS, h["df"][0] + Do)
        q = np.maximum(0.0, h["df"][0] * np.expm1(2.0 * (h["h"][0] - entry.astype(np.float64)) / (h["df"][0] + Do)))
        sig = np.sqrt(((h["df"][0] + q) / (h["df"][0] + Do))[:, None] * h["V"][0].astype(np.float32).astype(np.float64)[None])
        for j in (0, 1, 3, 4):
            want = mean.mean.T.astype(np.float64) + sig * z[j]
            assert np.all(np.abs(qs.values[j].T - want) <= 2 * rc.ulp32(want)), j


def stats_ppf(levels, nu):
    from scipy import stats
    return stats.t.ppf(np.asarray(levels), nu)


@pytest.mark.parametrize("overlap", [True, False])
def test_low_df_cluster(score, overlap):
    """A cluster with df + D_o <= 2: `return_std` is refused, the CDF and the quantiles are not."""
    c = case(1, 1, 3, 33, overlap, True)
    data, y = np.ascontiguousarray(c["X"].T), np.ascontiguousarray(c["Y"].T)
    parent, reg = open_regressor(score, c)
    with parent, reg:
        with pytest.raises(ValueError):
            reg.predict(data, return_std=True)
        res = reg.cdf(data, y)
        qs = reg.quantile(data, rc.LEVELS)
        _, probs = reg.marginal.predict(data)
        h = held(reg, c["X"])
    assert h["df"][0] + 1 <= 2
    ref = ref_cdf(h, probs, c["Y"])
    assert worst(res.cdf.T, ref["cdf"], ref["b_cdf"]) <= 1.0 and worst(res.sf.T, ref["sf"], ref["b_sf"]) <= 1.0
    for j, lv in enumerate(rc.LEVELS):
        err, bound = rc.quantile_contract(probs, h["B"], h["c"], h["V"], h["df"], h["q"], h["x"], qs.values[j].T, lv, t=h["t"])
        assert np.all(err <= bound)


@pytest.mark.parametrize("Do,Dt,K", [(5, 31, 3), (33, 130, 3)])
def test_bits_do_not_depend_on_how_the_work_is_cut(pkg, score, Do, Dt, K):
    import torch
    binding = importlib.import_module(pkg.__name__ + ".binding")
    n = 229
    c = case(Do, Dt, K, n)
    data, y = np.ascontiguousarray(c["X"].T), np.ascontiguousarray(c["Y"].T)
    perm = np.random.default_rng(5).permutation(n)
    runs = []
    for cap, budget in ((32, None), (64, None), (n, None), (1000, 4e-3)):
        parent, reg = open_regressor(score, c, capacity=cap)
        with parent, reg:
            if budget:
                reg.marginal._wk.set_option(binding.OPT_SCORE_TABLE_MB, budget)      # a range is one tile of the sweep
            runs.append((reg.cdf(data, y), reg.quantile(data, rc.LEVELS)))
            if cap == 64:
                before = reg.predict(data)
                p_cdf, p_q = reg.cdf(np.ascontiguousarray(data[:, perm]), np.ascontiguousarray(y[:, perm])), reg.quantile(np.ascontiguousarray(data[:, perm]), rc.LEVELS)
                d_cdf = reg.cdf(torch.as_tensor(data, device="cuda:0"), torch.as_tensor(y, device="cuda:0").double())
                d_q = reg.quantile(torch.as_tensor(data, device="cuda:0"), rc.LEVELS)
                alone = [reg.quantile(data, [lv]) for lv in (rc.LEVELS[1], rc.LEVELS[4])]
                shuffled = reg.quantile(data, (0.95, 0.3, 0.05))
                lower, upper = reg.interval(data, 0.9)
                after = reg.predict(data)
    a_cdf, a_q = runs[0]
    for o_cdf, o_q in runs[1:] + [(d_cdf, d_q)]:
        assert np.array_equal(bits(a_cdf.cdf), bits(o_cdf.cdf)) and np.array_equal(bits(a_cdf.sf), bits(o_cdf.sf)) and np.array_equal(bits(a_q.values), bits(o_q.values))
        assert np.array_equal(to_np(o_cdf.labels), a_cdf.labels)
    assert isinstance(d_cdf.cdf, torch.Tensor) and d_cdf.cdf.device == torch.device("cuda:0") and tuple(d_q.values.shape) == (5, Dt, n)
    assert np.array_equal(bits(a_cdf.cdf[:, perm]), bits(p_cdf.cdf)) and np.array_equal(bits(a_q.values[:, :, perm]), bits(p_q.values))
    assert np.array_equal(bits(alone[0].values[0]), bits(a_q.values[1])) and np.array_equal(bits(alone[1].values[0]), bits(a_q.values[4]))
    assert np.array_equal(bits(shuffled.values[0]), bits(a_q.values[3])) and np.array_equal(bits(shuffled.values[2]), bits(a_q.values[1]))
    assert np.array_equal(bits(lower), bits(a_q.values[1])) and np.array_equal(bits(upper), bits(a_q.values[3]))
    assert np.array_equal(bits(before.mean), bits(after.mean))


def test_skipped_points_nan_and_infinite_y(score):
    c = case(5, 31, 3, 33)
    X, Y = c["X"].copy(), c["Y"].copy()
    X[4, 2] = np.nan
    X[32, 0] = np.inf
    Y[7, 3] = np.nan
    Y[8, 0], Y[8, 1] = np.inf, -np.inf
    data, y = np.ascontiguousarray(X.T), np.ascontiguousarray(Y.T)
    parent, reg = open_regressor(score, c)
    with parent, reg:
        res, qs, pred = reg.cdf(data, y), reg.quantile(data, (0.5,)), reg.predict(data)
        clean = reg.cdf(np.ascontiguousarray(c["X"].T), np.ascontiguousarray(c["Y"].T))
    assert res.skipped == pred.skipped == qs.skipped == 2 and np.array_equal(res.labels, pred.labels) and np.array_equal(qs.labels, pred.labels)
    for i in (4, 32):
        assert np.isnan(res.cdf[:, i]).all() and np.isnan(res.sf[:, i]).all() and np.isnan(qs.values[:, :, i]).all()
    assert np.isnan(res.cdf[3, 7]) and np.isnan(res.sf[3, 7])
    assert res.cdf[0, 8] == 1.0 and res.sf[0, 8] == 0.0 and res.cdf[1, 8] == 0.0 and res.sf[1, 8] == 1.0
    keep = np.ones((31, 33), bool)
    keep[:, [4, 32]] = False
    keep[3, 7] = keep[0, 8] = keep[1, 8] = False
    assert np.array_equal(bits(res.cdf)[keep], bits(clean.cdf)[keep]) and not np.isnan(res.cdf[keep]).any() and not np.isnan(qs.values[0][:, [7, 8]]).any()


def law_model(score):
    """A model over D = 6 features with K = 4 overlapping clusters, and 20000 points drawn from its own joint."""
    L = rc.LAW
    post = rc.law_posterior()
    model = rr.dummy_model(post, L["K"], L["D"])
    with score.Predictor(model, capacity=L["n"]) as p:
        drawn = p.sample(L["n"], seed=L["seed"])
    pts = to_np(drawn.points if hasattr(drawn, "points") else drawn[0])
    return model, np.ascontiguousarray(pts, np.float32)


def test_law_pit_values_are_uniform(score):
    L = rc.LAW
    model, pts = law_model(score)
    assert pts.shape == (L["D"], L["n"])
    with score.Predictor(model, capacity=4096) as p, p.regressor(L["given"], L["targets"]) as reg:
        res = reg.cdf(np.ascontiguousarray(pts[L["given"]]), np.ascontiguousarray(pts[L["targets"]]))
        _, probs = reg.marginal.predict(np.ascontiguousarray(pts[L["given"]]))
    assert res.skipped == 0 and float(((probs != 0).sum(1) > 1).mean()) > 0.5
    for d in range(len(L["targets"])):
        dist = rc.kolmogorov(res.cdf[d])
        print(f"target {d}: Kolmogorov distance of the PIT values {dist:.5f} < {L['limit']:.5f}")
        assert dist < L["limit"]


def test_quantiles_agree_with_the_draws(score):
    """A handful of points of the one-target model, 4000 draws each: the empirical CDF of a point's draws at its returned quantiles is
    within the Kolmogorov criterion for 4000 draws (one sample per point; the criterion bounds the empirical CDF everywhere, so also at
    the three quantiles)."""
    c = case(1, 1, 3, 33)
    data = np.ascontiguousarray(c["X"].T[:, :5])
    m = 4000
    parent, reg = open_regressor(score, c)
    with parent, reg:
        qs = reg.quantile(data, (0.05, 0.5, 0.95))
        draws = reg.sample(data, draws=m, seed=11).values                # (m, 1, 5)
        _, probs = reg.marginal.predict(data)
    assert ((probs != 0).sum(1) > 1).any()
    emp = (draws[:, None, :, :] <= qs.values[None, :, :, :]).mean(0)      # (3, 1, 5)
    dist = np.abs(emp - np.array([0.05, 0.5, 0.95])[:, None, None]).max()
    print(f"empirical CDF of 4000 draws at the quantiles: worst distance {dist:.5f} < {1.63 / np.sqrt(m):.5f}")
    assert dist < 1.63 / np.sqrt(m)


def test_absorb_refreshes_both_calls_and_one_shots(pkg, score):
    c = case(5, 31, 3, 33)
    data, y = np.ascontiguousarray(c["X"].T), np.ascontiguousarray(c["Y"].T)
    mod = importlib.import_module(score.__name__.rsplit(".", 1)[0])
    model = rr.dummy_model(c["post"], c["K"], c["D"])
    one = mod.regress_cdf(model, data, y, c["given"], c["targets"], capacity=CAP)
    oneq = mod.regress_quantile(model, data, c["given"], c["targets"], levels=(0.05, 0.95), capacity=CAP)
    parent, reg = open_regressor(score, c)
    with parent, reg:
        a, aq = reg.cdf(data, y), reg.quantile(data, (0.05, 0.95))
        assert np.array_equal(bits(a.cdf), bits(one.cdf)) and np.array_equal(bits(aq.values), bits(oneq.values))
        reg.marginal.absorb(np.ascontiguousarray(data[:, :20] + 0.5))
        b, bq = reg.cdf(data, y), reg.quantile(data, (0.05, 0.95))
        _, probs = reg.marginal.predict(data)
        h = held(reg, c["X"])
    assert not np.array_equal(bits(a.cdf), bits(b.cdf)) and not np.array_equal(bits(aq.values), bits(bq.values))
    ref = ref_cdf(h, probs, c["Y"])
    assert worst(b.cdf.T, ref["cdf"], ref["b_cdf"]) <= 1.0
    for j, lv in enumerate((0.05, 0.95)):
        err, bound = rc.quantile_contract(probs, h["B"], h["c"], h["V"], h["df"], h["q"], h["x"], bq.values[j].T, lv, t=h["t"])
        assert np.all(err <= bound)
