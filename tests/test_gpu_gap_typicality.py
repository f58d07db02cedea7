"""GPU tests of DPMM_OPT_TYPICALITY_GAPS (typ_gap_kernel of csrc/typicality.hip, explain_gap_kernel of csrc/explain_gap.hip) and of the `gaps=`
keyword of Predictor.typicality / Predictor.explain: a point with NaN gaps is scored and explained under the marginal of its own cluster's
Student-t over the features it has.

The reference is numpy Float64 (tests/tools/gap_typicality_ref.py, checked on the CPU by tests/test_gap_typicality_cpu.py); its docstring
states the bounds the results are held to, which are those of include/dpmm_hip_typicality.h and include/dpmm_hip_explain.h.  Tails are
compared as tests/test_gpu_typicality.py and tests/test_gpu_explain.py compare theirs: against the Float64 tail of the RETURNED q / z-score,
relative 2^-20 wherever that is at least 1e-30.  Models are written by hand (K = 3, df = D + 3), n = 600 points in slabs of 256 (two cuts, a
short last slab); every third point has gaps, point 5 has more gaps than the cap and point 8 a gap and +Inf in an observed feature."""
import importlib
import os

import numpy as np
import pytest
import torch

import test_gpu_explain as GE
from tools import explain_ref as E
from tools import gap_typicality_ref as G
from tools import poison
from tools import typicality_ref as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, K, CAP = 600, 3, 256
TAIL_REL = 2.0 ** -20
ROWS = GE.ROWS
same, as_np = GE.same, GE.as_np


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def binding(pkg):
    return importlib.import_module(pkg.__name__ + ".binding")


@pytest.fixture(scope="module")
def host(pkg):
    return importlib.import_module(pkg.__name__ + ".host")


def patterns(D, r):
    """The gap positions: feature 0, feature D - 1, both sides of lane 63 / 64, spread over the tiles."""
    cap = min(16, D - 1)
    if r == "1":
        pats = [[0], [D - 1], [D // 2]] + ([[63], [64]] if D > 64 else [])
    elif r == "2":
        pats = [[0, D - 1], [1, D // 2 + 1]] + ([[63, 64], [62, 63], [64, 65]] if D > 65 else [[63, 64]] if D == 65 else [])
    else:
        pats = [np.unique(np.linspace(0, D - 1, cap).astype(int)).tolist(), list(range(cap)), list(range(D - cap, D))]
        pats = [q for q in pats if len(q) == cap]
        pats += [list(range(56, 56 + cap))] if D > 72 else []
    return [np.asarray(q, np.int64) for q in pats]


def data(D, r, seed, n=N, k=K):
    """(post, X (D, n) Float32 with gaps, gappy: the indices of the points that are to be scored with gaps)."""
    rng = np.random.default_rng(seed)
    post, m, A, df = GE.model(D, k, D + 3.0, seed)
    X = GE.points(m, A, n, rng)
    pats = patterns(D, r)
    gappy = np.arange(k + 1, n, 3)
    gappy = gappy[(gappy != 5) & (gappy != 8)]
    for c, i in enumerate(gappy):
        X[pats[c % len(pats)], i] = np.nan
    X[:, 5] = np.nan                                                     # more gaps than the cap: skipped
    X[pats[0], 8] = np.nan                                               # a gap, and +Inf in an observed feature: never scored
    X[[j for j in range(D) if j not in set(pats[0].tolist())][0], 8] = np.inf
    return post, X, gappy


def check_tails(got, ref, what):
    big = ref >= 1e-30
    rel = np.abs(got[big] - ref[big]) / ref[big]
    print(what, "largest relative tail error in units of 2^-20:", float(rel.max() * 2 ** 20) if big.any() else 0.0)
    assert np.all(rel <= TAIL_REL) and np.all(got[~big] <= 1e-29) and np.all((got >= 0) & (got <= 1)), what


@pytest.mark.parametrize("r", ["1", "2", "cap"])
@pytest.mark.parametrize("D", [5, 64, 65, 130, 200, 256])
def test_values_classes_and_nothing_else_moves(host, D, r):
    post, X, gappy = data(D, r, 31 * D + len(r))
    what = ("D", D, "r", r)
    with GE.open_predictor(host, post, CAP, missing="marginalize") as p:
        params = GE.worker_params(p)
        d0, e0 = p.typicality(X), p.explain(X)
        g = p.typicality(X, gaps="marginalize")                          # on the parent commit: an unknown keyword
        full = p.explain(X, gaps="marginalize")
        tops = {mm: p.explain(X, top=mm, gaps="marginalize") for mm in sorted({min(4, D), min(16, D)})}
        d1, e1 = p.typicality(X), p.explain(X)
        labels = p.predict_labels(X)
        counts = p.missing_counts
    # ---- nothing else moves: the default call before and after, the labels, the complete points
    assert all(same(a, b) for a, b in zip(d0[:3], d1[:3])) and d0[3:] == d1[3:] and GE.same_exp(e0, e1), what
    assert same(g.labels, labels) and same(d0.labels, labels) and same(full.labels, labels) and counts == (len(gappy) + 1, 1), what
    q, tail, q0 = as_np(g.mahalanobis), as_np(g.tail), as_np(d0.mahalanobis)
    complete = ~np.isnan(X).any(0) & np.isfinite(X).all(0)
    assert np.isnan(q0[gappy]).all() and not np.isnan(q0[complete]).any(), what
    assert same(q[complete], q0[complete]) and same(tail[complete], as_np(d0.tail)[complete]), what
    for name in ROWS:
        assert same(as_np(getattr(full, name))[:, complete], as_np(getattr(e0, name))[:, complete]), (what, name)
    # ---- classes and counters
    assert not np.isnan(q[gappy]).any() and not np.isnan(tail[gappy]).any(), what      # NaN on the parent commit: the points are incomplete there
    assert np.isnan(tail[5]) and np.isnan(tail[8]) and np.isnan(q[5]) and np.isnan(q[8]), what
    assert g.skipped == d0.skipped and g.incomplete == d0.incomplete - len(gappy) and g.skipped >= 1, what
    assert int(np.isnan(tail).sum()) == g.skipped + g.incomplete == 2 and int(np.isnan(as_np(d0.tail)).sum()) == d0.skipped + d0.incomplete, what
    assert all(same(a, b) for a, b in zip(full[:3], g[:3])) and full[7:] == g[3:], what
    # ---- values of the points with gaps
    lab0 = as_np(g.labels)[gappy] - 1
    ref = G.reference(X[:, gappy], lab0, *params)
    err = np.abs(q[gappy].astype(np.float64) - ref.q) / ref.q_bound
    print(what, "largest error of q_o in units of its bound:", float(err.max()))
    assert np.all(err <= 1.0), what
    df64 = params[2].astype(np.float64)[lab0]
    check_tails(tail[gappy].astype(np.float64), T.tail_of(q[gappy], df64, D - ref.r), what + ("tail",))
    e, t, ft = (as_np(getattr(full, name))[:, gappy].T.astype(np.float64) for name in ROWS)
    mis = np.isnan(X[:, gappy].T)
    assert all(np.array_equal(np.isnan(a), mis) for a in (e, t, ft)), what                 # NaN exactly on M
    obs = ~mis
    re_, rt = np.abs(e - ref.e)[obs] / ref.e_bound[obs], np.abs(t - ref.t)[obs] / (2 * ref.t_bound[obs])
    print(what, "largest error in units of its bound: residual", float(re_.max()), "zscore (twice the first-order bound)", float(rt.max()))
    assert np.all(re_ <= 1.0) and np.all(rt <= 1.0), what
    dof = np.broadcast_to((df64 + D - ref.r - 1)[:, None], t.shape)
    check_tails(ft[obs], E.feature_tail_of(t[obs], dof[obs]), what + ("feature_tail",))
    # ---- top mode.  Against the kernel's own full result: the features of largest |zscore|, a missing one last and reported as -1, the
    # same bits gathered -- stricter than the reference can be, ties included.  Against the reference: position j holds the reference's
    # j-th feature wherever that feature's |zscore| is further from every other observed one's than the two bounds together (twice the
    # first-order bound each, as the values above).
    tt = as_np(full.zscore).T
    scored = ~np.isnan(q)
    ra_, rb = np.where(mis, -np.inf, np.abs(ref.t)), np.where(mis, 0.0, 2 * ref.t_bound)
    rorder = np.argsort(-ra_, axis=1, kind="stable")
    rows = np.arange(len(gappy))
    for mm, top in tops.items():
        feats = as_np(top.features)
        held = 0
        for j in range(mm):
            d = rorder[:, j]
            v, b = ra_[rows, d], rb[rows, d]
            live = np.isfinite(v)                                            # (position j of a point with D_o <= j holds a missing feature)
            apart = np.abs(np.where(live, v, 0.0)[:, None] - ra_) > b[:, None] + rb
            apart[rows, d] = True
            sep = live & apart.all(1)
            held += int(sep.sum())
            assert np.array_equal(feats[gappy][sep, j], d[sep]), (what, mm, j)
        print(what, "top", mm, "positions held to the reference's order:", held, "of", mm * len(gappy))
        want = np.argsort(-np.abs(tt), axis=1, kind="stable")[:, :mm]                      # (NaN sorts last)
        gone = np.isnan(np.take_along_axis(tt, want, 1)) & np.take_along_axis(np.isnan(X.T), want, 1)
        assert np.array_equal(feats[scored], np.where(gone, -1, want)[scored]) and np.all(feats[~scored] == -1), (what, mm)
        for name in ROWS:
            a, b = as_np(getattr(full, name)).T, as_np(getattr(top, name))
            assert same(np.take_along_axis(a, want, 1)[scored], b[scored]) and np.isnan(b[~scored]).all(), (what, mm, name)
        assert all(same(a, b) for a, b in zip(full[:3], top[:3])) and full[7:] == top[7:], (what, mm)
        if mm > D - 1:
            assert np.all(feats[gappy][:, -1] == -1), (what, mm)


@pytest.mark.parametrize("D,r", [(5, "cap"), (130, "2")])
def test_bits_do_not_depend_on_capacity_budget_or_order(host, binding, D, r):
    post, X, gappy = data(D, r, 77 * D)
    m = min(4, D)

    def run(p, Y):
        return p.typicality(Y, gaps="marginalize"), p.explain(Y, gaps="marginalize"), p.explain(Y, top=m, gaps="marginalize")
    with GE.open_predictor(host, post, CAP, missing="marginalize") as p:
        base = run(p, X)
        xd = torch.from_numpy(np.ascontiguousarray(X.T)).to(DEV).T       # a device tensor: full slabs read in place
        dev = run(p, xd)
    with GE.open_predictor(host, post, N, missing="marginalize") as p:  # one slab; then ranges of one tile; then the points reversed
        one = run(p, X)
        p._wk.set_option(binding.OPT_SCORE_TABLE_MB, 4e-3)
        tiles = run(p, X)
        p._wk.set_option(binding.OPT_SCORE_TABLE_MB, 1.0)
        back = run(p, np.ascontiguousarray(X[:, ::-1]))
    for other in (dev, one, tiles):
        assert all(same(a, b) for a, b in zip(base[0][:3], other[0][:3])) and base[0][3:] == other[0][3:]
        assert GE.same_exp(base[1], other[1]) and GE.same_exp(base[2], other[2])
    assert all(same(as_np(a)[::-1], b) for a, b in zip(base[0][:3], back[0][:3])) and base[0][3:] == back[0][3:]
    for i in (1, 2):
        assert all(same(as_np(a)[::-1], b) for a, b in zip(base[i][:3], back[i][:3]))
        assert all(same(as_np(a)[:, ::-1] if i == 1 else as_np(a)[::-1], b) for a, b in zip(base[i][3:7], back[i][3:7]) if a is not None)


def test_impute_then_score_has_the_same_q_and_a_larger_tail(host):
    """K = 1: the imputed point sits at the conditional mean of its gaps, so its complete-case q is q_o -- within the sum of the two bounds --
    but its tail is judged at D degrees of freedom instead of D - r and comes out LARGER: why imputing first is the wrong workaround."""
    D = 12
    post, X, gappy = data(D, "2", 5, n=300, k=1)
    with GE.open_predictor(host, post, CAP, missing="marginalize") as p:
        params = GE.worker_params(p)
        g = p.typicality(X, gaps="marginalize")
        filled = p.impute(X)
        f = p.typicality(filled)
    ref = G.reference(X[:, gappy], np.zeros(len(gappy), np.int64), *params)
    _, af, _ = T.reference(as_np(filled)[:, gappy], np.zeros(len(gappy), np.int64), *params)
    # q as a function of the missing features is q_o + (x_M - x*)' A_MM (x_M - x*) around the conditional mean x*: the Float32 rounding of the
    # filled features and the error of t enter in second order only, below ((D + 3) u)^2 (a + a_x) with a_x = sum_r (sum_{c in M} |R_rc| |x_c|)^2
    qg, qf = as_np(g.mahalanobis)[gappy].astype(np.float64), as_np(f.mahalanobis)[gappy].astype(np.float64)
    u = 2.0 ** -24
    xm = np.where(np.isnan(X[:, gappy]), np.abs(as_np(filled)[:, gappy].astype(np.float64)), 0.0)
    ax = ((np.abs(params[1][0].astype(np.float64)) @ xm) ** 2).sum(0)
    bound = ref.q_bound + (3 * D + 4) * u * af + ((D + 3) * u) ** 2 * (af + ax)
    print("largest |q(impute) - q_o| in units of the summed bounds:", float((np.abs(qg - qf) / bound).max()))
    assert np.all(np.abs(qg - qf) <= bound)
    tg, tf = as_np(g.tail)[gappy], as_np(f.tail)[gappy]
    far = qg > 1e-3
    assert far.sum() > 50 and np.all(tf[far] > tg[far])


def test_tails_of_points_with_gaps_are_uniform(host):
    """20000 draws of the model itself with 1 .. 4 random features knocked out (D = 8): `tail` and `feature_tail` of feature 0, which is kept,
    are uniform on (0, 1): Kolmogorov distance below 1.63 / sqrt(n), the criterion of tests/test_gpu_typicality.py."""
    D, n = 8, 20000
    post, m, A, df = GE.model(D, K, D + 3.0, 11)
    rng = np.random.default_rng(12)
    with GE.open_predictor(host, post, 8192, missing="marginalize") as p:
        X = np.array(as_np(p.sample(n, seed=3)[0]), np.float32)         # (D, n)
        for i in range(n):
            X[1 + rng.choice(D - 1, rng.integers(1, 5), replace=False), i] = np.nan
        ex = p.explain(X, gaps="marginalize")
    tail, ft = as_np(ex.tail).astype(np.float64), as_np(ex.feature_tail)[0].astype(np.float64)
    assert ex.skipped == ex.incomplete == 0 and not np.isnan(tail).any() and not np.isnan(ft).any()
    d1, d2 = T.ks_uniform(tail), T.ks_uniform(ft)
    print("Kolmogorov distances (tail, feature_tail of feature 0):", d1, d2, "criterion", 1.63 / np.sqrt(n))
    assert d1 < 1.63 / np.sqrt(n) and d2 < 1.63 / np.sqrt(n)


@pytest.mark.parametrize("pattern", [0xffffffff, 0x7fc00000])
def test_results_ignore_lds_and_register_contents(host, pattern):
    """The gap kernels read LDS only where their own wave wrote it: the same bits with the LDS and the register files refilled first."""
    if not os.path.exists(poison.SO) and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("tests/tools/libpoison.so is not built and there is no hipcc to build it with")
    poison.build()                                                       # (a failure of the build itself fails the test)
    post, X, gappy = data(130, "cap", 9)
    out = []
    with GE.open_predictor(host, post, N, missing="marginalize") as p:
        for dirty in (False, True):
            if dirty:
                poison.poison(pattern)
            a = p.typicality(X, gaps="marginalize")
            if dirty:
                poison.poison(pattern)
            b = p.explain(X, top=16, gaps="marginalize")
            if dirty:
                poison.poison(pattern)
            out.append((a, b, p.explain(X, gaps="marginalize")))
    (a0, b0, c0), (a1, b1, c1) = out
    assert all(same(x, y) for x, y in zip(a0[:3], a1[:3])) and a0[3:] == a1[3:] and GE.same_exp(b0, b1) and GE.same_exp(c0, c1)
