"""GPU tests of mixture regression (include/dpmm_hip_regress.h, csrc/regress.hip) through host/score.py's Predictor.marginal, Regressor
and regress.

The reference is tests/tools/regress_ref.py (Float64, checked on the CPU by tests/test_condition_cpu.py: a second independent form, five
planted mistakes outside the bound): every entry of mean and std must lie within the header's bound, evaluated from the Float32
probabilities the GPU returned, the Float64 tables and -- for the term the table entry puts on s_ik -- predictive_ref.error_bound.
Shapes: regress_ref.CASES, n = two 32-point tiles + 5, run in slabs of 40 points, with the planted points regress_ref.make_case lists.

Measured on an MI355X, worst got / bound per case (printed by the tests): see DESIGN section 29.
"""
import functools
import importlib
import os
import tempfile

import numpy as np
import pytest

from tools import missing_ref as mr
from tools import predictive_ref as pr
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
def case(Do, Dt, K):
    return rr.make_case(Do, Dt, K)


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def to_np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def open_regressor(score, c, capacity=CAP, **kw):
    parent = score.Predictor(rr.dummy_model(c["post"], c["K"], c["D"]), capacity=capacity, **kw)
    return parent, parent.regressor(c["given"], c["targets"])


def reference_for(reg, probs, X, **kw):
    """regress_ref.reference on what the worker holds: the tables, the marginal model's Float32 parameters, the probabilities returned."""
    B, cc, V, h, df = reg.tables()
    m, R, logdet, dff, w = (np.asarray(a, np.float32) for a in reg.marginal._predictive_args()[1])
    K, Do = m.shape
    want, parts = pr.student_t_table(X, m, R, logdet, dff, w)
    parts["want"] = want
    t = pr.error_bound(X, m, R, dff, parts).T
    return rr.reference(probs, B, cc, V, df, parts["q"].T, X.astype(np.float64), t=t, m_O=m.astype(np.float64), **kw), h, parts


def worst(got, want, bound):
    fin = np.isfinite(want)
    assert np.isfinite(got[fin]).all()
    return float((np.abs(got[fin].astype(np.float64) - want[fin]) / bound[fin]).max())


@pytest.mark.parametrize("Do,Dt,K", rr.CASES)
def test_mean_and_std_against_float64(score, Do, Dt, K):
    c = case(Do, Dt, K)
    data = np.ascontiguousarray(c["X"].T)
    parent, reg = open_regressor(score, c)
    with parent, reg:
        res = reg.predict(data, return_std=True)
        plain = reg.predict(data)
        lab, probs = reg.marginal.predict(data)
        ref, h, parts = reference_for(reg, probs, c["X"])
    assert res.mean.shape == (Dt, c["n"]) and res.std.shape == (Dt, c["n"]) and res.mean.dtype == np.float32 and res.skipped == 0 and plain.std is None
    assert np.array_equal(bits(plain.mean), bits(res.mean)) and np.array_equal(res.labels, lab) and np.array_equal(plain.labels, lab)
    r_mean = worst(res.mean.T, ref["mean"], ref["mean_bound"])
    r_std = worst(res.std.T, ref["std"], ref["std_bound"])
    print(f"Do={Do} Dt={Dt} K={K}: worst got / bound: mean {r_mean:.3f}  std {r_std:.3f}")
    assert r_mean <= 1.0 and r_std <= 1.0
    pl = c["planted"]
    # a point at cluster 0's mean: where every other entry lies more than 110 below (expf underflows: with few given features the
    # Student-t tails are too heavy for that), the other probabilities are exactly 0 -- the clusters the kernel leaves out
    i = pl["alone"]
    gone = bool(np.all(parts["want"][1:, i] - parts["want"][0, i] < -110.0))
    assert gone or Do < 33 or K == 1
    if gone:
        assert probs[i, 0] == 1.0 and not probs[i, 1:].any()
    if K >= 2:
        # the balanced point between clusters 0 and 1: its std exceeds both components' own
        i = pl["mid"]
        assert probs[i, 0] > 0.05 and probs[i, 1] > 0.05
        B, cc, V, _, df = reg.tables()
        own = np.sqrt((df[:2, None] + parts["q"][:2, i][:, None]) / (df[:2, None] + Do - 2) * V[:2])
        assert np.all(res.std[:, i] > own.max(0))
        # the cluster 1e4 standard deviations out, the Float32 cancellation case: the bound is not vacuous there (it grows with
        # D_o |x|: checked where the given features are few)
        if Do <= 16:
            for i in pl["far"]:
                assert np.all(ref["std_bound"][i] < 0.5 * ref["std"][i]), (ref["std_bound"][i] / ref["std"][i]).max()


@pytest.mark.parametrize("Do,Dt", [(3, 2), (64, 64)])
def test_one_cluster_closed_form(score, Do, Dt):
    c = case(Do, Dt, 1)
    data = np.ascontiguousarray(c["X"].T)
    parent, reg = open_regressor(score, c)
    with parent, reg:
        res = reg.predict(data, return_std=True)
        _, probs = reg.marginal.predict(data)
        ref, _, parts = reference_for(reg, probs, c["X"])
        _, _, V, _, df = reg.tables()
    want = np.sqrt((df[0] + parts["q"][0])[:, None] / (df[0] + Do - 2) * V[0][None, :])
    assert np.all(np.abs(res.std.T - want) <= ref["std_bound"])


@pytest.mark.parametrize("Do,Dt,K", [(3, 2, 3), (65, 63, 3), (64, 64, 24)])
def test_bits_do_not_depend_on_capacity_budget_or_input_kind(pkg, score, Do, Dt, K):
    import torch
    binding = importlib.import_module(pkg.__name__ + ".binding")
    c = case(Do, Dt, K)
    data = np.ascontiguousarray(c["X"].T)
    parent, reg = open_regressor(score, c)
    with parent, reg:
        a = reg.predict(data, return_std=True)
        lab = reg.marginal.predict_labels(data)
        dev = reg.predict(torch.as_tensor(data, device="cuda:0"), return_std=True)
        wide = torch.zeros((c["n"], 2 * Do + 1), dtype=torch.bfloat16, device="cuda:0")
        wide[:, ::2][:, :Do] = torch.as_tensor(c["X"], device="cuda:0").to(torch.bfloat16)
        strided = wide[:, ::2][:, :Do].T                                   # (D_o, n) bfloat16, both strides odd ones out
        assert not strided.is_contiguous() and not strided.T.is_contiguous()
        b16 = reg.predict(strided, return_std=True)
        b32 = reg.predict(strided.float().contiguous(), return_std=True)
    parent, reg = open_regressor(score, c, capacity=1000)
    with parent, reg:
        reg.marginal._wk.set_option(binding.OPT_SCORE_TABLE_MB, 4e-3)     # a range is one tile of the sweep
        b = reg.predict(data, return_std=True)
    assert isinstance(dev.mean, torch.Tensor) and dev.mean.device == torch.device("cuda:0") and tuple(dev.mean.shape) == (Dt, c["n"])
    for other in (b, dev):
        assert np.array_equal(bits(a.mean), bits(other.mean)) and np.array_equal(bits(a.std), bits(other.std))
        assert np.array_equal(to_np(other.labels), lab) and other.skipped == 0
    assert np.array_equal(a.labels, lab)
    assert np.array_equal(bits(b16.mean), bits(b32.mean)) and np.array_equal(bits(b16.std), bits(b32.std)) and torch.equal(b16.labels, b32.labels)


def test_skipped_points(score):
    c = case(33, 31, 3)
    X = c["X"].copy()
    planted = {rr.TILE - 1: np.nan, rr.TILE: np.inf, 2 * rr.TILE + 4: -np.inf, CAP - 1: np.nan}
    for i, v in planted.items():
        X[i, (7 * i) % c["Do"]] = v
    parent, reg = open_regressor(score, c)
    with parent, reg:
        base = reg.predict(np.ascontiguousarray(c["X"].T), return_std=True)
        got = reg.predict(np.ascontiguousarray(X.T), return_std=True)
    rows = np.array(sorted(planted))
    keep = np.setdiff1d(np.arange(c["n"]), rows)
    assert got.skipped == len(planted) and base.skipped == 0
    assert np.isnan(got.mean[:, rows]).all() and np.isnan(got.std[:, rows]).all()
    assert np.array_equal(bits(got.mean[:, keep]), bits(base.mean[:, keep])) and np.array_equal(bits(got.std[:, keep]), bits(base.std[:, keep]))


@pytest.mark.parametrize("D,r", [(5, 1), (5, 2), (64, 1), (64, 16)])
def test_marginal_model_and_mean_agree_with_the_gap_path(pkg, score, D, r):
    """Two independent routes to the same numbers: marginal(O) on X[O] against the Predictor(missing="marginalize") on the same points with
    the targets set to NaN, and the regression mean against what `impute` writes into those gaps."""
    c = rr.make_case(D - r, r, 3)
    O, M = c["given"], c["targets"]
    full = np.full((c["n"], D), np.nan, np.float32)
    full[:, O] = c["X"]
    with score.Predictor(rr.dummy_model(c["post"], 3, D), capacity=CAP, missing="marginalize") as parent:
        reg = parent.regressor(O, M)
        with reg:
            ld_gap = parent.score_samples(np.ascontiguousarray(full.T))
            lab_gap, p_gap = parent.predict(np.ascontiguousarray(full.T))
            filled = parent.impute(np.ascontiguousarray(full.T))
            data = np.ascontiguousarray(c["X"].T)
            ld = reg.marginal.score_samples(data)
            lab, p = reg.marginal.predict(data)
            res = reg.predict(data)
            ref, _, parts = reference_for(reg, p, c["X"])
            # the gap path's own tolerances, from its Float64 reference on the parameters its worker holds
            m, R, logdet, df, w = (np.asarray(a, np.float32) for a in parent._predictive_args()[1])
            gref = mr.reference(full, m, R.reshape(3, D, D), logdet, df, w)
            der = mr.derived(gref)
            mm, Rm, ldm, dfm, wm = (np.asarray(a, np.float32) for a in reg.marginal._predictive_args()[1])
            want, mparts = pr.student_t_table(c["X"], mm, Rm, ldm, dfm, wm)
            tb = pr.error_bound(c["X"], mm, Rm, dfm, mparts, rounded_R=True)      # (both workers hold Float32 roundings of one Float64 model)
    assert gref["check"].all()
    tol_ld = der["ld_tol"] + tb.max(0) + 2.0 ** -23 * (3 + 16) + 2.0 ** -23 * np.abs(ld.astype(np.float64))
    tol_p = der["p_tol"] + p.astype(np.float64) * (np.expm1(2 * tb.max(0)) + 2.0 ** -23 * (3 + 16))[:, None]
    assert np.all(np.abs(ld.astype(np.float64) - ld_gap) <= tol_ld) and np.all(np.abs(p.astype(np.float64) - p_gap) <= tol_p)
    differ = np.flatnonzero(lab != lab_gap)
    best2 = np.sort(want, axis=0)[-2:]
    assert np.all(best2[1, differ] - best2[0, differ] <= (gref["bound"].max(0) + tb.max(0))[differ] * 2)
    worst_fill = 0.0
    for i in range(c["n"]):
        v = filled[M, i]
        worst_fill = max(worst_fill, float((np.abs(v.astype(np.float64) - res.mean[:, i]) / (_fill_tol(der, gref, i, M) + ref["mean_bound"][i])).max()))
    print(f"D={D} r={r}: regression mean against impute, worst difference / (sum of the two bounds) {worst_fill:.3f}")
    assert worst_fill <= 1.0


def _fill_tol(der, gref, i, M):
    """missing_ref lists a point's gaps in increasing feature order: its tolerances in the order of the targets M."""
    order = {int(f): j for j, f in enumerate(np.flatnonzero(gref["miss"][i]))}
    return np.array([der["fill_tol"][int(i)][order[int(f)]] for f in M])


def test_state_absorb_and_save_load(pkg, score):
    binding = importlib.import_module(pkg.__name__ + ".binding")
    c = case(16, 17, 3)
    data = np.ascontiguousarray(c["X"].T)
    # ---- the worker: regress before the tables are set, and after the parameters moved
    parent, reg = open_regressor(score, c)
    with parent, reg:
        wk = pkg.Worker(0, c["Do"], CAP)
        try:
            wk.set_predictive_niw(*reg.marginal._predictive_args()[1])
            wk.upload_points(np.ascontiguousarray(c["X"][:CAP]))
            mean = np.empty((CAP, c["Dt"]), np.float32)
            with pytest.raises(binding.DpmmError) as e:
                wk.regress_points_into(mean)
            assert e.value.code == ESTATE
            wk.set_regression(*reg.tables()[:4])
            wk.regress_points_into(mean)
            wk.set_predictive_niw(*reg.marginal._predictive_args()[1])
            with pytest.raises(binding.DpmmError) as e:
                wk.regress_points_into(mean)
            assert e.value.code == ESTATE
        finally:
            wk.close()
        before = reg.predict(data)
        assert np.array_equal(bits(before.mean[:, :CAP]), bits(mean.T))
        # ---- absorb: the tables are refreshed, the means move to the new model's reference
        mid = c["planted"]["mid"]
        batch = np.ascontiguousarray(np.repeat(c["X"][mid:mid + 1], 64, axis=0).T)
        reg.marginal.absorb(batch)
        after = reg.predict(data)
        _, probs = reg.marginal.predict(data)
        ref, _, _ = reference_for(reg, probs, c["X"])
        assert worst(after.mean.T, ref["mean"], ref["mean_bound"]) <= 1.0
        assert not np.array_equal(bits(after.mean[:, mid]), bits(before.mean[:, mid]))
    # ---- save / load: the marginal model round-trips; a Regressor rebuilt from the loaded parent gives the same bits
    parent, reg = open_regressor(score, c)
    with parent, reg, tempfile.TemporaryDirectory() as d:
        first = reg.predict(data, return_std=True)
        ld = reg.marginal.score_samples(data)
        reg.marginal.save(os.path.join(d, "marginal.npz"))
        parent.save(os.path.join(d, "parent.npz"))
        with score.Predictor.load(os.path.join(d, "marginal.npz"), capacity=CAP) as m2:
            assert m2.D == c["Do"] and np.array_equal(bits(m2.score_samples(data)), bits(ld))
        with score.Predictor.load(os.path.join(d, "parent.npz"), capacity=CAP) as p2, p2.regressor(c["given"], c["targets"]) as r2:
            again = r2.predict(data, return_std=True)
    assert np.array_equal(bits(first.mean), bits(again.mean)) and np.array_equal(bits(first.std), bits(again.std))


def test_one_shot_form(pkg, score):
    host = importlib.import_module(pkg.__name__ + ".host")
    c = case(3, 2, 3)
    data = np.ascontiguousarray(c["X"].T)
    parent, reg = open_regressor(score, c)
    with parent, reg:
        a = reg.predict(data, return_std=True)
    b = host.regress(rr.dummy_model(c["post"], 3, c["D"]), data, c["given"], c["targets"], return_std=True, capacity=CAP)
    assert np.array_equal(bits(a.mean), bits(b.mean)) and np.array_equal(bits(a.std), bits(b.std)) and b.skipped == 0
