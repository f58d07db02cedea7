"""GPU tests of the draws of the targets (include/dpmm_hip_regress_draw.h, csrc/regress_draw.hip) through host/score.py's Regressor.sample
and regress_sample, and through the binding.

The reference is tests/tools/regress_draw_ref.py (Float64, from the same random words; checked on the CPU by
tests/test_regress_draws_cpu.py: two independent sides, the planted mistakes outside the bound, the law): every drawn value must lie
within its bound, the components must be the reference's but for the excused draws (at most 1 %), and the law test runs on the GPU's own
values.  Shapes: regress_ref.CASES, n = two 32-point tiles + 5 with overlapping clusters, run in slabs of 40 points.
"""
import ctypes
import functools
import importlib

import numpy as np
import pytest

from tools import predictive_ref as pr
from tools import regress_draw_ref as rd
from tools import regress_ref as rr

pytestmark = pytest.mark.gpu

CAP = 40
ESTATE = -4      # DPMM_ESTATE (include/dpmm_hip.h)


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


@functools.lru_cache(maxsize=None)
def case(Do, Dt, K, n=rd.N):
    return rd.make_case(Do, Dt, K, n=n)


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def to_np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def open_regressor(score, c, capacity=CAP, **kw):
    parent = score.Predictor(rr.dummy_model(c["post"], c["K"], c["D"]), capacity=capacity, **kw)
    return parent, parent.regressor(c["given"], c["targets"])


def held(reg, X):
    """What the worker holds: the joint model, df, the marginal table in Float64 and the bound of its entries."""
    m, R = reg._joint_parameters()
    mm, Rm, ld, dff, w = (np.asarray(a, np.float32) for a in reg.marginal._predictive_args()[1])
    want, parts = pr.student_t_table(X, mm, Rm, ld, dff, w)
    parts["want"] = want
    t = pr.error_bound(X, mm, Rm, dff, parts).T
    return dict(m=m, R=R, df=dff.astype(np.float64), want=want, t=t, q=parts["q"].T)


def against_reference(reg, X, res, seed, idx=None):
    h = held(reg, X)
    n, K = X.shape[0], len(h["df"])
    vals, comp = to_np(res.values).transpose(0, 2, 1), to_np(res.components)
    ref = rd.draw(X, h["m"], h["R"], h["df"], h["want"], np.arange(n) if idx is None else idx, vals.shape[0], seed, comp=comp, t=h["t"], q=h["q"])
    return rd.compare(vals, comp, ref, rd.relative_table_error(h["t"], K)) + (ref,)


@pytest.mark.parametrize("Do,Dt,K", rd.CASES)
def test_draws_against_float64(score, Do, Dt, K):
    c = case(Do, Dt, K)
    seed = rd.case_seed(Do, Dt, K)
    data = np.ascontiguousarray(c["X"].T)
    parent, reg = open_regressor(score, c)
    with parent, reg:
        res = reg.sample(data, draws=3, seed=seed, return_components=True)
        lab = reg.marginal.predict_labels(data)
        ratio, exc, wrong, ref = against_reference(reg, c["X"], res, seed)
    assert res.values.shape == (3, Dt, c["n"]) and res.values.dtype == np.float32 and res.components.shape == (3, c["n"]) and res.skipped == 0
    assert np.array_equal(res.labels, lab)
    print(f"Do={Do} Dt={Dt} K={K}: worst got / bound {ratio:.3f}, excused {exc:.4f}, components wrong {wrong}, "
          f"components in tile 0: {len(np.unique(res.components[:, :rd.TILE]))}")
    assert ratio <= 1.0 and exc <= rd.MAX_EXCUSED and wrong == 0
    if K > 1:
        assert len(np.unique(res.components[:, :rd.TILE])) > 1


@pytest.mark.parametrize("Do,Dt", rd.LAW_SHAPES)
def test_law_on_the_gpu_values(score, Do, Dt):
    c = case(Do, Dt, 1, rd.LAW_POINTS)
    data = np.ascontiguousarray(c["X"].T)
    parent, reg = open_regressor(score, c, capacity=rd.LAW_POINTS)
    with parent, reg:
        res = reg.sample(data, draws=rd.LAW_DRAWS, seed=rd.LAW_SEED[(Do, Dt)])
        h = held(reg, c["X"])
    tb = rd.tables(h["m"], h["R"], Do)
    X64 = c["X"].astype(np.float64)
    mu = tb["c"][0][None] + X64 @ tb["B"][0].T
    z = X64 - tb["m_O"][0][None]
    q = np.einsum("ne,ef,nf->n", z, tb["Soo_inv"][0], z)
    stat = rd.law_statistic(to_np(res.values).transpose(0, 2, 1), mu, tb["S"][0], h["df"][0], q, Do)
    assert stat.size == 16384
    d, lim = rd.check_law(stat, Dt, h["df"][0] + Do)
    print(f"Do={Do} Dt={Dt}: KS distance {d:.5f} < {lim:.5f}")


def test_pooled_moments_against_the_closed_form(score):
    """One cluster, D = 8 with the last 3 features the targets, 64 draws x 256 points: the whitened residuals u = W^-1 (x - mu) / sqrt((df + q) /
    (df + D_o)) are t_{df + D_o} with identity scale; their pooled mean and covariance lie within five standard errors of 0 and
    dfo / (dfo - 2) I (a coordinate's variance has relative variance 2 (dfo - 1) / ((dfo - 4) N), a correlation (dfo - 2) / ((dfo - 4) N))."""
    c = rd.make_case(5, 3, 1, n=256, scramble=False)
    c["post"]["nu"][:] = 30.0 + c["D"] - 1            # df = 30
    data = np.ascontiguousarray(c["X"].T)
    parent, reg = open_regressor(score, c, capacity=256)
    with parent, reg:
        res = reg.sample(data, draws=64, seed=5)
        h = held(reg, c["X"])
    tb = rd.tables(h["m"], h["R"], 5)
    X64 = c["X"].astype(np.float64)
    mu = tb["c"][0][None] + X64 @ tb["B"][0].T
    z = X64 - tb["m_O"][0][None]
    q = np.einsum("ne,ef,nf->n", z, tb["Soo_inv"][0], z)
    dfo = h["df"][0] + 5
    r = to_np(res.values).transpose(0, 2, 1).astype(np.float64) - mu[None]
    u = np.linalg.solve(tb["W"][0], r.reshape(-1, 3).T).T.reshape(r.shape) / np.sqrt((h["df"][0] + q) / dfo)[None, :, None]
    u = u.reshape(-1, 3)
    N = len(u)
    var = dfo / (dfo - 2.0)
    assert np.all(np.abs(u.mean(0)) <= 5 * np.sqrt(var / N))
    C = np.cov(u.T)
    assert np.all(np.abs(np.diag(C) / var - 1) <= 5 * np.sqrt(2 * (dfo - 1) / ((dfo - 4) * N)))
    corr = C / np.sqrt(np.outer(np.diag(C), np.diag(C)))
    assert np.all(np.abs(corr[np.triu_indices(3, 1)]) <= 5 * np.sqrt((dfo - 2) / ((dfo - 4) * N)))


@pytest.mark.parametrize("Do,Dt,K", [(3, 2, 3), (65, 63, 3), (64, 64, 24)])
def test_bits_do_not_depend_on_how_the_work_is_cut(pkg, score, Do, Dt, K):
    import torch
    binding = importlib.import_module(pkg.__name__ + ".binding")
    c = case(Do, Dt, K)
    n = c["n"]
    data = np.ascontiguousarray(c["X"].T)
    parent, reg = open_regressor(score, c)
    with parent, reg:
        before = reg.predict(data, return_std=True)
        a = reg.sample(data, draws=4, seed=9, return_components=True)
        again = reg.sample(data, draws=4, seed=9, return_components=True)
        after = reg.predict(data, return_std=True)
        dev = reg.sample(torch.as_tensor(data, device="cuda:0"), draws=4, seed=9, return_components=True)
        b16 = reg.sample(torch.as_tensor(data, device="cuda:0").to(torch.bfloat16), draws=2, seed=9)
        b32 = reg.sample(torch.as_tensor(data, device="cuda:0").to(torch.bfloat16).float(), draws=2, seed=9)
        # draw0-split calls through the binding, on the first slab
        wk = reg.marginal._wk
        wk.upload_points(np.ascontiguousarray(c["X"][:CAP]))
        one = np.empty((CAP, 4, Dt), np.float32)
        wk.regress_draw_points_into(one, 9, 0)
        lo, hi = np.empty((CAP, 1, Dt), np.float32), np.empty((CAP, 3, Dt), np.float32)
        wk.regress_draw_points_into(lo, 9, 0, draw0=0)
        wk.regress_draw_points_into(hi, 9, 0, draw0=1)
        # a permuted data set with the indices kept: the slab's points in a random order; position j holds point perm[j], and the call with
        # i0 = BASE + perm[j] - j gives position j the global index BASE + perm[j] -- one call per position, its row kept
        BASE = 100
        straight = np.empty((CAP, 4, Dt), np.float32)
        wk.regress_draw_points_into(straight, 9, BASE)
        perm = np.random.default_rng(3).permutation(CAP)
        assert not np.array_equal(perm, np.arange(CAP))
        wk.upload_points(np.ascontiguousarray(c["X"][:CAP][perm]))
        permuted, scratch = np.empty((CAP, 4, Dt), np.float32), np.empty((CAP, 4, Dt), np.float32)
        for j in range(CAP):
            wk.regress_draw_points_into(scratch, 9, BASE + int(perm[j]) - j)
            permuted[j] = scratch[j]
    for cap in (n, 32, 33):
        parent, reg = open_regressor(score, c, capacity=cap)
        with parent, reg:
            if cap == 33:
                reg.marginal._wk.set_option(binding.OPT_SCORE_TABLE_MB, 4e-3)     # a range is one tile of the sweep
            b = reg.sample(data, draws=4, seed=9, return_components=True)
        assert np.array_equal(bits(a.values), bits(b.values)) and np.array_equal(a.components, b.components) and b.skipped == 0
    assert np.array_equal(bits(a.values), bits(again.values)) and np.array_equal(a.components, again.components)
    assert np.array_equal(bits(before.mean), bits(after.mean)) and np.array_equal(bits(before.std), bits(after.std))
    assert isinstance(dev.values, torch.Tensor) and dev.values.device == torch.device("cuda:0") and tuple(dev.values.shape) == (4, Dt, n)
    assert np.array_equal(bits(a.values), bits(dev.values)) and np.array_equal(a.components, to_np(dev.components)) and np.array_equal(a.labels, to_np(dev.labels))
    assert np.array_equal(bits(b16.values), bits(b32.values))
    av = np.ascontiguousarray(a.values.transpose(2, 0, 1))                # (n, draws, D_t)
    assert np.array_equal(bits(one), bits(av[:CAP])) and np.array_equal(bits(lo), bits(av[:CAP, :1])) and np.array_equal(bits(hi), bits(av[:CAP, 1:]))
    assert np.array_equal(bits(permuted), bits(straight[perm])) and not np.array_equal(bits(straight), bits(one))


def test_skipped_points(score):
    c = case(33, 31, 3)
    X = c["X"].copy()
    planted = {rd.TILE - 1: np.nan, rd.TILE: np.inf, 2 * rd.TILE + 4: -np.inf, CAP - 1: np.nan}
    for i, v in planted.items():
        X[i, (7 * i) % c["Do"]] = v
    parent, reg = open_regressor(score, c)
    with parent, reg:
        base = reg.sample(np.ascontiguousarray(c["X"].T), draws=3, seed=4, return_components=True)
        got = reg.sample(np.ascontiguousarray(X.T), draws=3, seed=4, return_components=True)
    rows = np.array(sorted(planted))
    keep = np.setdiff1d(np.arange(c["n"]), rows)
    assert got.skipped == len(planted) and base.skipped == 0
    assert np.isnan(got.values[:, :, rows]).all() and (got.components[:, rows] == -1).all()
    assert np.array_equal(bits(got.values[:, :, keep]), bits(base.values[:, :, keep])) and np.array_equal(got.components[:, keep], base.components[:, keep])


def test_row_without_a_finite_entry(pkg, score):
    """A point so far out that its quadratic forms overflow in Float32: every entry of its row of the worker's table is -Inf (the worker's own
    log-density says so), and it takes no part; the other points of its tile keep their bits."""
    c = case(3, 2, 3)
    X = c["X"].copy()
    X[5] = 3e38
    parent, reg = open_regressor(score, c)
    with parent, reg:
        base = reg.sample(np.ascontiguousarray(c["X"].T), draws=2, seed=4, return_components=True)
        got = reg.sample(np.ascontiguousarray(X.T), draws=2, seed=4, return_components=True)
        ld = reg.marginal.score_samples(np.ascontiguousarray(X.T))
        _, probs = reg.marginal.predict(np.ascontiguousarray(X.T))
    assert ld[5] == -np.inf and np.isfinite(np.delete(ld, 5)).all(), ld[5]
    assert not np.isfinite(probs[5]).all() or not probs[5].any()
    keep = np.arange(c["n"]) != 5
    assert got.skipped == 1 and base.skipped == 0
    assert np.isnan(got.values[:, :, 5]).all() and (got.components[:, 5] == -1).all()
    assert np.array_equal(bits(got.values[:, :, keep]), bits(base.values[:, :, keep])) and np.array_equal(got.components[:, keep], base.components[:, keep])


def test_components_agree_with_impute_draws(score):
    """D = 8 with the last 3 features NaN: `impute(draws=m)` and `Regressor.sample` pick their components from the same probabilities by
    the same rule, each with the uniforms of its own stream (43 and 46).  Fed those uniforms, the rule (impute_draw_ref.pick on the Float64
    probabilities) gives the components of either call, but for the draws excused by that call's own table error."""
    from tools import impute_draw_ref as idr
    from tools import missing_ref as mr
    D, r, K, m, seed = 8, 3, 3, 8, 21
    c = rd.make_case(D - r, r, K, scramble=False)
    n = c["n"]
    full = np.full((n, D), np.nan, np.float32)
    full[:, :D - r] = c["X"]
    idx = np.arange(n)
    with score.Predictor(rr.dummy_model(c["post"], K, D), capacity=CAP, missing="marginalize") as parent:
        with parent.regressor(c["given"], c["targets"]) as reg:
            _, comp_i = parent.impute(np.ascontiguousarray(full.T), draws=m, seed=seed, return_components=True)
            res = reg.sample(np.ascontiguousarray(c["X"].T), draws=m, seed=seed, return_components=True)
            h = held(reg, c["X"])
            pm, pR, pld, pdf, pw = (np.asarray(a, np.float32) for a in parent._predictive_args()[1])
    gref = mr.reference(full, pm, pR.reshape(K, D, D), pld, pdf, pw)
    with np.errstate(all="ignore"):
        rel_i = np.expm1(2 * gref["bound"].max(0)) + mr.EPS * (K + 16)
    rel_r = rd.relative_table_error(h["t"], K)
    p_i, p_r = idr.probabilities(gref["want"]), idr.probabilities(h["want"])
    assert np.abs(p_i - p_r).max() <= 1e-5                                  # (two Float32 roundings of one Float64 model)
    wrong_i = wrong_r = exc = same = 0
    for j in range(m):
        u_i, u_r = idr.uniform(idx, j, seed), rd.uniform(idx, j, seed)
        own_i, own_r = idr.pick(p_i, u_i)[0], idr.pick(p_r, u_r)[0]
        e_i, e_r = idr.excused(p_i, u_i, rel_i), idr.excused(p_r, u_r, rel_r)
        wrong_i += int(((comp_i[j] != own_i) & ~e_i).sum())
        wrong_r += int(((res.components[j] != own_r) & ~e_r).sum())
        exc += int(e_i.sum() + e_r.sum())
        # the same uniforms give the same components: the rule applied to the OTHER call's uniforms gives the other call's components
        same += int(((idr.pick(p_r, u_i)[0] != comp_i[j]) & ~e_i & ~idr.excused(p_r, u_i, rel_r)).sum())
    assert wrong_i == 0 and wrong_r == 0 and same == 0 and exc <= rd.MAX_EXCUSED * 2 * m * n, (wrong_i, wrong_r, same, exc)
    assert len(np.unique(res.components)) > 1 and len(np.unique(comp_i)) > 1


def test_state_and_absorb(pkg, score):
    binding = importlib.import_module(pkg.__name__ + ".binding")
    c = case(16, 17, 3)
    data = np.ascontiguousarray(c["X"].T)
    parent, reg = open_regressor(score, c)
    with parent, reg:
        wk = pkg.Worker(0, c["Do"], CAP)
        try:
            wk.set_predictive_niw(*reg.marginal._predictive_args()[1])
            wk.upload_points(np.ascontiguousarray(c["X"][:CAP]))
            out = np.empty((CAP, 2, c["Dt"]), np.float32)
            tabs = reg.tables(factor=True)
            wk.set_regression(*tabs[:4])
            with pytest.raises(binding.DpmmError) as e:
                wk.regress_draw_points_into(out, 1, 0)
            assert e.value.code == ESTATE
            wk.set_regression_factor(tabs[5])
            wk.regress_draw_points_into(out, 1, 0)
            wk.set_regression(*tabs[:4])                     # new tables: the factor goes with the old ones
            with pytest.raises(binding.DpmmError) as e:
                wk.regress_draw_points_into(out, 1, 0)
            assert e.value.code == ESTATE
        finally:
            wk.close()
        before = reg.sample(data, draws=2, seed=1, return_components=True)
        assert np.array_equal(bits(before.values[:, :, :CAP]), bits(out.transpose(1, 2, 0)))
        B0, c0, _, h0, _, W0 = reg.tables(factor=True)
        batch = np.ascontiguousarray(np.repeat(c["X"][5:6], 64, axis=0).T)
        reg.marginal.absorb(batch)
        B1, c1, _, h1, _, W1 = reg.tables(factor=True)
        assert np.array_equal(B0, B1) and np.array_equal(c0, c1) and np.array_equal(W0, W1) and not np.array_equal(h0, h1)
        after = reg.sample(data, draws=2, seed=1, return_components=True)
        ratio, exc, wrong, _ = against_reference(reg, c["X"], after, 1)
        assert ratio <= 1.0 and wrong == 0 and exc <= rd.MAX_EXCUSED
        assert not np.array_equal(bits(after.values), bits(before.values))


def test_one_table_evaluation_for_all_draws(pkg, score):
    """The kernel launches of an m-draw call on one range are those of a one-draw call: the table is evaluated once, not once per draw."""
    c = case(3, 2, 3)
    lib = ctypes.CDLL(pkg.lib_path())
    count = [0]
    HOOK = ctypes.CFUNCTYPE(None, ctypes.c_void_p)
    cb = HOOK(lambda _: count.__setitem__(0, count[0] + 1))
    parent, reg = open_regressor(score, c, capacity=CAP)
    with parent, reg:
        wk = reg.marginal._wk
        wk.upload_points(np.ascontiguousarray(c["X"][:CAP]))
        launches = []
        lib.dpmm_debug_set_prelaunch_hook.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.dpmm_debug_set_prelaunch_hook(ctypes.cast(cb, ctypes.c_void_p), None)
        try:
            for m in (1, 7):
                count[0] = 0
                wk.regress_draw_points_into(np.empty((CAP, m, c["Dt"]), np.float32), 3, 0)
                launches.append(count[0])
        finally:
            lib.dpmm_debug_set_prelaunch_hook(None, None)
    assert launches[0] > 0 and launches[0] == launches[1], launches


def test_one_shot_form(pkg, score):
    host = importlib.import_module(pkg.__name__ + ".host")
    c = case(3, 2, 3)
    data = np.ascontiguousarray(c["X"].T)
    parent, reg = open_regressor(score, c)
    with parent, reg:
        a = reg.sample(data, draws=3, seed=11, return_components=True)
    b = host.regress_sample(rr.dummy_model(c["post"], 3, c["D"]), data, c["given"], c["targets"], draws=3, seed=11, return_components=True, capacity=CAP)
    assert np.array_equal(bits(a.values), bits(b.values)) and np.array_equal(a.components, b.components) and b.skipped == 0
