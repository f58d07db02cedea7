"""GPU tests of missing features (include/dpmm_hip_missing.h, csrc/missing.hip) through host/score.py's Predictor.

The reference is tests/tools/missing_ref.py (Float64, checked on the CPU by tests/test_missing_cpu.py: two independent forms, a restatement
inside the bound, seven planted mistakes outside it): per table entry a bound derived from Float64 quantities alone, and from it -- not
chosen -- the tolerances of what users see:
    log-density     max_k bound_k + 2^-23 (K + 16) + 2^-23 |want|        the finish kernel's term of tests/test_gpu_score.py
    probabilities   p_k (expm1(2 max_k bound_k) + 2^-23 (K + 16))
    top-m           the j-th largest probability moves by at most the largest of those (order statistics are 1-Lipschitz)
    label           a cluster whose entry is within bound_label + bound_best of the best one
    imputed value   sum_k p_k dcm_k + sum_k p_k rel |c_k - v| + 2^-23 |v|  (missing_ref's docstring)
Shapes: predictive_ref.make_case's n = 2 tiles + 5 for D = 2, 5, 16, 17, 33, 64, 65, 128, 256 at K = 3 and (24, 60), with the gaps
missing_ref.make_case plants (first and last position, both sides of the tile boundary, r = 1, 2, cap, 17, D, NaN with +Inf, a cluster mean
with a gap), run in slabs of 40 points (7 or 13 slabs, the one at 80 .. 119 without a gap); plus missing_ref.make_correlated_case
(cond(Sigma) about 4e4: the case that tells a Float64 residual from a Float32 difference).
Everything a complete point gets is compared BIT FOR BIT with missing="propagate".

Measured on an MI355X, worst got / tolerance per case (printed by the tests): see DESIGN section 18.
"""
import contextlib
import functools
import importlib
import types

import numpy as np
import pytest

from tools import missing_ref as mr

pytestmark = pytest.mark.gpu

CAP = 40
CORRELATED = ("correlated", 3)


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def score(pkg):
    return importlib.import_module(pkg.__name__ + ".host.score")


@functools.lru_cache(maxsize=None)
def case_ref(D, K):
    """(case, reference, derived tolerances): computed once, shared, never modified."""
    c = mr.make_correlated_case() if (D, K) == CORRELATED else mr.make_case(D, K)
    ref = mr.reference(c["X"], c["m"], c["R"], c["logdet"], c["df"], c["w"])
    return c, ref, mr.derived(ref)


def dummy_model(D, K):
    """What a Predictor reads of a fitted model; the worker below is handed the case's own parameters instead of its conversion."""
    post = dict(kappa=np.ones(3 * K), nu=np.full(3 * K, D + 3.0), m=np.zeros((3 * K, D)), U=np.tile(np.eye(D), (3 * K, 1, 1)), logdet_psi=np.zeros(3 * K))
    s = types.SimpleNamespace(K=K, prior=types.SimpleNamespace(kind=0, dim=D), post=post, alpha=10.0, points_count=np.full(K, 10), wk=types.SimpleNamespace(device=0))
    return types.SimpleNamespace(sampler=s)


def predictor(pkg, score, c, missing, capacity=CAP):
    class CaseWorker(pkg.Worker):
        def set_predictive_niw(self, m, R, logdet, df, weights):
            super().set_predictive_niw(c["m"], c["R"].reshape(c["K"], -1), c["logdet"], c["df"], c["w"])
    return score.Predictor(dummy_model(c["D"], c["K"]), capacity=capacity, worker_factory=CaseWorker, missing=missing)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def outputs(p, data, m):
    ld = p.score_samples(data)
    counts = [p.missing_counts]
    lab, probs = p.predict(data)
    counts.append(p.missing_counts)
    lab2, idx, tp = p.predict_topk(data, m)
    counts.append(p.missing_counts)
    to = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)      # noqa: E731
    return dict(ld=to(ld), lab=to(lab), probs=to(probs), lab2=to(lab2), idx=to(idx), tp=to(tp)), counts


def same_bits(a, b, rows):
    return all(np.array_equal(bits(a[k][rows]) if a[k].dtype == np.float32 else a[k][rows], bits(b[k][rows]) if b[k].dtype == np.float32 else b[k][rows])
               for k in a)


CASES = mr.CASES + (CORRELATED,)


@pytest.mark.parametrize("D,K", CASES)
def test_marginal_scores_against_float64(pkg, score, D, K):
    c, ref, der = case_ref(D, K)
    n, Kc = c["n"], c["K"]
    data = np.ascontiguousarray(c["X"].T)
    m = min(Kc, 3)
    planted = (int(ref["listed"].sum()), int(ref["over"].sum()))
    assert n > 2 * CAP and planted[0] >= 8
    if "free_slab" in c:
        assert not (ref["listed"] | ref["over"])[c["free_slab"][0]:c["free_slab"][1]].any() and c["free_slab"][0] % CAP == 0
    with predictor(pkg, score, c, "marginalize") as p:
        got, counts = outputs(p, data, m)
    with predictor(pkg, score, c, "propagate") as p:
        base, counts0 = outputs(p, data, m)
    assert counts == [planted] * 3 and counts0 == [(0, 0)] * 3
    # ---- complete points: bit for bit what they get without the option
    complete = ref["r"] == 0
    assert same_bits(got, base, complete)
    # ---- over the cap: the all-NaN row stays
    over = ref["over"]
    # (the log-density of an all-NaN row is -Inf by dpmm_hip_score.h's definition, its probabilities NaN, its label "the first NaN")
    assert np.isneginf(got["ld"][over]).all() and np.isnan(got["probs"][over]).all() and np.all(got["lab"][over] == 1) and same_bits(got, base, over)
    # ---- NaN with +Inf: marginalised, and as non-finite as an Inf feature makes a point
    if "naninf" in c:
        assert ref["listed"][c["naninf"]] and not np.isfinite(got["ld"][c["naninf"]])
    # ---- marginalised points against Float64
    chk = np.flatnonzero(ref["check"])
    assert np.isneginf(base["ld"][chk]).all() and np.isnan(base["probs"][chk]).all() and np.isfinite(got["ld"][chk]).all()
    r_ld = np.abs(got["ld"][chk] - der["logdens"][chk]) / der["ld_tol"][chk]
    r_p = np.abs(got["probs"][chk] - der["probs"][chk]) / der["p_tol"][chk]
    want_sorted = -np.sort(-der["probs"][chk], axis=1)[:, :m]
    r_top = np.abs(got["tp"][chk] - want_sorted) / der["p_tol"][chk].max(1, keepdims=True)
    print(f"D={D} K={K}: {len(chk)} marginalised points, worst got / tolerance: logdens {r_ld.max():.3f}  probs {r_p.max():.3f}  top-{m} {r_top.max():.3f}")
    assert r_ld.max() <= 1.0 and r_p.max() <= 1.0 and r_top.max() <= 1.0
    want, bound = ref["want"][:, chk], ref["bound"][:, chk]
    best = want.argmax(0)
    lab0 = got["lab"][chk] - 1
    cols = np.arange(len(chk))
    assert np.all(want[lab0, cols] >= want[best, cols] - bound[lab0, cols] - bound[best, cols])
    assert np.array_equal(got["lab"], got["lab2"]) and np.array_equal(bits(got["tp"][chk]), bits(np.take_along_axis(got["probs"][chk], got["idx"][chk] - 1, 1)))


@pytest.mark.parametrize("D,K", [(5, 3), (64, 3), (128, 3)])
def test_results_do_not_depend_on_capacity_or_table_budget(pkg, score, D, K):
    binding = importlib.import_module(pkg.__name__ + ".binding")
    c, ref, _ = case_ref(D, K)
    data = np.ascontiguousarray(c["X"].T)
    with predictor(pkg, score, c, "marginalize") as p:
        a, _ = outputs(p, data, 2)
        fa = p.impute(data)
    with predictor(pkg, score, c, "marginalize", capacity=c["n"] - 3) as p:
        p._wk.set_option(binding.OPT_SCORE_TABLE_MB, 4e-3)                      # a range is one tile of the sweep
        b, counts = outputs(p, data, 2)
        fb = p.impute(data)
        assert p.missing_counts == counts[0] == (int(ref["listed"].sum()), int(ref["over"].sum()))
    assert same_bits(a, b, slice(None)) and np.array_equal(bits(fa), bits(fb))


def test_data_without_gaps_is_bit_identical(pkg, score):
    c = dict(case_ref(64, 3)[0])
    X = np.where(np.isnan(c["X"]), np.float32(0.25), c["X"])
    data = np.ascontiguousarray(X.T)
    with predictor(pkg, score, c, "marginalize") as p:
        a, counts = outputs(p, data, 2)
        ex_a = p.exemplars(data, 4)
        fill = p.impute(data)
    with predictor(pkg, score, c, "propagate") as p:
        b, _ = outputs(p, data, 2)
        ex_b = p.exemplars(data, 4)
    assert counts == [(0, 0)] * 3 and same_bits(a, b, slice(None)) and np.array_equal(bits(fill), bits(data))
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(ex_a[:5], ex_b[:5])) and ex_a.skipped == ex_b.skipped


@pytest.mark.parametrize("D,K", CASES)
def test_impute_against_float64(pkg, score, D, K):
    import torch
    c, ref, der = case_ref(D, K)
    data = np.ascontiguousarray(c["X"].T)
    with predictor(pkg, score, c, "propagate") as p:                           # works whether or not the option is set
        got = p.impute(data)
        assert p.missing_counts == (int(ref["listed"].sum()), int(ref["over"].sum()))
        dev = p.impute(torch.as_tensor(data, device="cuda:0"))
        ints = (torch.arange(c["D"] * 100, device="cuda:0").reshape(c["D"], 100) % 7 - 3).to(torch.int16)      # no NaN in an integer type: converted
        dev16 = p.impute(ints)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == data.shape
    assert isinstance(dev, torch.Tensor) and dev.device == torch.device("cuda:0") and dev.dtype == torch.float32 and tuple(dev.shape) == data.shape
    assert np.array_equal(bits(dev.cpu().numpy()), bits(got))
    assert dev16.dtype == torch.float32 and torch.equal(dev16, ints.float())
    gaps = np.isnan(data)
    assert np.array_equal(bits(got)[~gaps], bits(data)[~gaps])                 # observed features and complete points: bit for bit
    assert np.isnan(got[:, ref["over"]][gaps[:, ref["over"]]]).all()           # over the cap: the gaps stay
    worst = 0.0
    for i in np.flatnonzero(ref["check"]):
        v = got[ref["miss"][i], i]
        assert np.isfinite(v).all(), i
        worst = max(worst, float((np.abs(v - der["fill"][int(i)]) / der["fill_tol"][int(i)]).max()))
    print(f"D={D} K={K}: imputed values, worst got / tolerance {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("D,K", [(16, 3), (64, 3), (65, 3)])
def test_exemplars_rank_a_marginalised_point_at_a_cluster_mean_among_the_most_typical(pkg, score, D, K):
    c, ref, _ = case_ref(D, K)
    data = np.ascontiguousarray(c["X"].T)
    w = np.where(np.isnan(ref["want"]), -np.inf, ref["want"])                  # in Float64 the point is the best of its cluster, by a margin
    mine = np.flatnonzero((w.argmax(0) == c["k0"]) & (np.arange(c["n"]) != c["mean_gap"]))
    assert w[:, c["mean_gap"]].argmax() == c["k0"] and w[c["k0"], c["mean_gap"]] > w[c["k0"], mine].max() + 1.0
    with predictor(pkg, score, c, "marginalize") as p:
        ex = p.exemplars(data, 3, which="typical")
        assert p.missing_counts == (int(ref["listed"].sum()), int(ref["over"].sum()))
    with predictor(pkg, score, c, "propagate") as p:
        ex0 = p.exemplars(data, 3, which="typical")
    assert ex.typical_idx[c["k0"]][0] == c["mean_gap"] and c["mean_gap"] not in ex0.typical_idx.ravel().tolist()
    assert c["naninf"] not in ex.typical_idx.ravel().tolist()
    assert ex0.skipped - ex.skipped == int(ref["check"].sum()) and ex.skipped >= int(ref["over"].sum()) + 1      # (+ 1: the NaN with +Inf point)
    assert int(ex.count.sum()) + ex.skipped == c["n"]


def test_nothing_depends_on_what_earlier_kernels_left_in_lds_or_registers(pkg, score):
    """The list, patch and impute kernels with LDS and the register files refilled with a NaN pattern in front of every launch
    (tests/tools/poison.py through DPMM_LAUNCH's hook): the same bits."""
    from tools import poison
    poison.build()                      # (a build failure is a failure here, not a skip)
    binding = importlib.import_module(pkg.__name__ + ".binding")
    c, _, _ = case_ref(65, 3)
    data = np.ascontiguousarray(c["X"].T)
    res = []
    for dirty in (False, True):
        with (poison.poisoned_kernel_launches(binding, 0xffffffff) if dirty else contextlib.nullcontext()) as launches:
            with predictor(pkg, score, c, "marginalize") as p:
                out, _ = outputs(p, data, 2)
                out["fill"] = p.impute(data)
        res.append(out)
    assert launches[0] > 20 and same_bits(res[0], res[1], slice(None))


def test_counts_speak_of_the_last_call_also_where_it_returns_early(pkg, score):
    c, ref, _ = case_ref(5, 3)
    data = np.ascontiguousarray(c["X"].T)
    with predictor(pkg, score, c, "marginalize") as p:
        p.score_samples(data)
        wk = p._wk
        assert wk.score_missing_counts()[0] > 0                                # the last slab holds position n - 1
        wk.rank_begin(2)
        wk.rank_accumulate(0, 0)                                               # nothing to rank: returns before it evaluates anything
        assert wk.score_missing_counts() == (0, 0)
        p.score_samples(data)
        with pytest.raises(pkg.DpmmError):
            wk.score_points_raw(False, m=1)                                    # an argument error (m > 0 without top_idx / top_prob)
        assert wk.score_missing_counts() == (0, 0)
