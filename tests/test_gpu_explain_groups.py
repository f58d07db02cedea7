"""GPU tests of include/dpmm_hip_explain_groups.h (csrc/explain_group.hip) and of host/score.py's Predictor.explain_groups.

The reference is numpy Float64 (tests/tools/explain_groups_ref.py, which also lists the cases) from the Float32 m, R, df the worker is
given.  Models are made through Predictor._setup from posteriors written by hand, no fit; K = 3, n = 300, capacity 128 (two slabs and a short
one), DPMM_OPT_SCORE_TABLE_MB = 0 (ranges of one tile).  The points are drawn by `Predictor.sample`, six of them then pushed far out along
the first group.  For every scored point of every case, with u = 2^-24 and the header's bounds:

  labels, mahalanobis, tail   the bits of `typicality`
  group_mahalanobis           |q_G - ref| <= 2 qg_bound
  group_tail                  against betainc at the f recomputed in numpy Float32 from the returned q, q_G, df: relative 2^-20 wherever
                              the reference is at least 1e-30; both at most 1e-29 below
  a group of one feature      group_tail and `explain`'s feature_tail both lie between the tails at the two ends of the union of the
                              intervals their bounds leave (f_G +- 2 f_bound, (|t_d| +- 2 t_bound)^2), widened by 2^-20
  the group of all features   group_tail and `tail` likewise (f_G +- 2 f_bound, q +- dq)."""
import importlib

import numpy as np
import pytest
import torch

import test_gpu_score as S
from tools import explain_groups_ref as EG
from tools import explain_ref as E
from tools import poison
from tools import typicality_ref as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TAIL_REL = 2.0 ** -20
N, K, CAP = EG.N_CASE, EG.K_CASE, 128


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


def as_np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def same(a, b):
    """Equal shapes, types and bits."""
    a, b = np.ascontiguousarray(as_np(a)), np.ascontiguousarray(as_np(b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_exp(a, b):
    return all(same(x, y) for x, y in zip(a[:5], b[:5])) and a[5:] == b[5:]


def open_predictor(host, post, cap, **kw):
    Kk, D = post["m"].shape
    p = host.Predictor.__new__(host.Predictor)
    p._setup(0, D, 10.0, np.full(Kk, 100.0), post, cap, 0, None, **kw)
    return p


def worker_params(p):
    which, (m, R, logdet, df, w) = p._predictive_args()
    return T.worker_params(m, R, df)


def drawn_points(p, m, A, groups, seed):
    """(D, n) Float32 on the host: `sample`'s draws, shuffled so that the slabs mix the clusters, six pushed far out along the first group."""
    xs, lab = p.sample(N, seed=seed)
    order = np.random.default_rng(seed).permutation(N)
    X = np.ascontiguousarray(as_np(xs)[:, order])
    return EG.push_out(X, as_np(lab)[order] - 1, m, A, groups)


def between(name, value, lo_stat, hi_stat, dof, s, what):
    """`value` (Float32 tails from the GPU) lies between the tails at hi_stat and lo_stat, widened by 2^-20; underflow as elsewhere."""
    hi = EG.tail_of(np.maximum(lo_stat, 0.0), dof, s) * (1 + TAIL_REL)
    lo = EG.tail_of(hi_stat, dof, s) * (1 - TAIL_REL)
    v = value.astype(np.float64)
    big = lo >= 1e-30
    assert np.all(v[big] >= lo[big]) and np.all(v[hi >= 1e-30] <= hi[hi >= 1e-30]) and np.all(v[hi < 1e-30] <= 1e-29), (what, name)


def check(got, typ, full, X, params, groups, what):
    """Every per-point assertion of the module's description; returns the scored mask."""
    D, n = X.shape
    G = len(groups)
    sizes = np.array([len(g) for g in groups])
    lab, q, tail = as_np(got.labels), as_np(got.mahalanobis), as_np(got.tail)
    gq, gt = as_np(got.group_mahalanobis), as_np(got.group_tail)
    assert all(same(x, y) for x, y in zip(got[:3], typ[:3])) and got[7:] == typ[3:], what                # typicality's values, to the bit
    assert gq.shape == gt.shape == (G, n) and gq.dtype == gt.dtype == np.float32 and got.sizes == tuple(sizes), what
    ok = ~np.isnan(q)
    assert int((~ok).sum()) == got.skipped + got.incomplete, what
    assert np.isnan(gq[:, ~ok]).all() and np.isnan(gt[:, ~ok]).all() and not np.isnan(gq[:, ok]).any() and not np.isnan(gt[:, ok]).any(), what
    lab0 = lab[ok] - 1
    ref = EG.reference(X[:, ok], lab0, *params, groups)
    gq, gt = gq[:, ok].T, gt[:, ok].T                                                                    # (n, G)
    frac = np.abs(gq - ref.qg) / np.maximum(2 * ref.qg_bound, 1e-300)
    df32 = params[2][lab0]
    f32 = EG.stat32(q[ok][:, None], gq, df32[:, None], D, sizes[None, :])                                # the bits of the kernel's f
    dof = df32.astype(np.float64)[:, None] + (D - sizes)[None, :]
    tr = EG.tail_of(f32.astype(np.float64), dof, sizes[None, :])
    big = tr >= 1e-30
    rel = np.abs(gt[big] - tr[big]) / tr[big]
    print(what, "group_mahalanobis: worst error in units of twice its bound", float(frac.max()), "| group_tail: worst relative error in units of 2^-20",
          float(rel.max() * 2 ** 20), "tails below 1e-30:", int((~big).sum()))
    assert np.all(np.abs(gq - ref.qg) <= 2 * ref.qg_bound), what
    assert np.all(rel <= TAIL_REL) and np.all(gt[~big] <= 1e-29) and np.all((gt >= 0) & (gt <= 1)), what
    assert np.all(gq <= q[ok][:, None] * (1 + 1e-3) + 1e-6), what                                        # q_-G >= 0 up to the bound's order
    wrong = EG.swapped(groups)
    if wrong is not None:                                                                                # the bound tells a wrong grouping apart on these points
        assert EG.discriminates(ref, EG.reference(X[:, ok], lab0, *params, wrong)), what
    f_lo, f_hi = ref.f - 2 * ref.f_bound, ref.f + 2 * ref.f_bound
    singles = [j for j, g in enumerate(groups) if len(g) == 1]
    if singles:                                                                                          # against explain's feature_tail
        feats = [groups[j][0] for j in singles]
        ft = as_np(full.feature_tail)[feats][:, ok].T
        er = E.reference(X[:, ok], lab0, *params)
        ta = np.abs(er.t[:, feats])
        t_lo, t_hi = np.maximum(ta - 2 * er.t_bound[:, feats], 0.0) ** 2, (ta + 2 * er.t_bound[:, feats]) ** 2
        lo, hi = np.minimum(f_lo[:, singles], t_lo), np.maximum(f_hi[:, singles], t_hi)
        d1 = dof[:, singles]
        print(what, len(singles), "groups of one feature: largest |group_tail - feature_tail| / feature_tail", float(np.nanmax(np.abs(gt[:, singles] - ft) / np.maximum(ft, 1e-30))))
        between("group_tail", gt[:, singles], lo, hi, d1, 1, what)
        between("feature_tail", ft, lo, hi, d1, 1, what)
    if G == 1 and sizes[0] == D:                                                                         # against tail
        _, ai, _ = T.reference(X[:, ok], lab0, *params)
        dq = (3 * D + 4) * E.U32 * ai
        lo, hi = np.minimum(f_lo[:, 0], ref.q - dq), np.maximum(f_hi[:, 0], ref.q + dq)
        d1 = df32.astype(np.float64)
        print(what, "the group of all features: largest |group_tail - tail| / tail", float(np.max(np.abs(gt[:, 0] - tail[ok]) / np.maximum(tail[ok], 1e-30))))
        between("group_tail", gt[:, 0], lo, hi, d1, D, what)
        between("tail", tail[ok], lo, hi, d1, D, what)
    return ok


# ------------------------------------------------------------------------------------------------ every case
@pytest.mark.parametrize("heavy", [True, False], ids=["df=D+3", "df=1e5"])
@pytest.mark.parametrize("case", EG.CASES, ids=EG.CASE_IDS)
def test_every_case(host, binding, case, heavy):
    D, name, groups = case
    post, m, A, df = EG.case_model(D, heavy)
    what = (name, "D", D, "df", float(df[0]))
    with open_predictor(host, post, CAP) as p:
        p._wk.set_option(binding.OPT_SCORE_TABLE_MB, 0.0)                                                # every slab in ranges of one tile
        params = worker_params(p)
        X = drawn_points(p, m, A, groups, 77 + D)
        typ = p.typicality(X)
        full = p.explain(X) if any(len(g) == 1 for g in groups) else None
        got = p.explain_groups(X, groups)
        ok = check(got, typ, full, X, params, groups, what)
        assert ok.all() and (got.skipped, got.incomplete) == (0, 0)
        far = as_np(got.group_tail)[0, -2:]                                                              # 30 units out along the first group
        assert np.all(far < 1e-6), (what, far)
        xd = torch.from_numpy(np.ascontiguousarray(X.T)).to(DEV).T                                       # a device tensor, full slabs read in place
        dgot = p.explain_groups(xd, groups)
        assert all(torch.is_tensor(v) and v.device == torch.device(DEV) for v in dgot[:5])
        assert same_exp(got, dgot)
    with open_predictor(host, post, N) as p:                                                             # one slab, the default budget
        one = p.explain_groups(X, {f"g{j}": g for j, g in enumerate(groups)})
    assert one.names == tuple(f"g{j}" for j in range(len(groups))) and got.names is None
    assert all(same(x, y) for x, y in zip(got[:5], one[:5])) and got[6:] == one[6:]


# ------------------------------------------------------------------------------------------------ the classes
def test_skipped_and_incomplete_points(host):
    D, n = 6, 300
    groups = [[0, 3], [1], [2, 4, 5]]
    post, m, A, df = EG.case_model(D, True)
    with open_predictor(host, post, CAP) as p:
        clean = drawn_points(p, m, A, groups, 5)
    X = clean.copy()
    X[0, 7] = np.nan                                                                                     # one gap
    X[2, 250] = np.nan
    X[1, 100] = np.inf                                                                                   # no finite entry in its row
    X[:, 290] = np.nan                                                                                   # nothing left to marginalise over
    gaps, lost = [7, 250], [100, 290]
    rest = np.setdiff1d(np.arange(n), gaps + lost)
    for missing, counts in (("propagate", (len(gaps) + len(lost), 0)), ("marginalize", (len(lost), len(gaps)))):
        with open_predictor(host, post, CAP, missing=missing) as p:
            base, got, typ = p.explain_groups(clean, groups), p.explain_groups(X, groups), p.typicality(X)
            assert (got.skipped, got.incomplete) == counts == typ[3:], missing                           # exactly as typicality counts them
            assert all(same(x, y) for x, y in zip(got[:3], typ[:3])), missing
            for a, c in ((as_np(got.group_mahalanobis), as_np(base.group_mahalanobis)), (as_np(got.group_tail), as_np(base.group_tail))):
                assert np.isnan(a[:, gaps + lost]).all() and same(a[:, rest], c[:, rest]) and not np.isnan(a[:, rest]).any(), missing


# ------------------------------------------------------------------------------------------------ the generation of the tables
def test_tables_of_an_older_predictive_are_refused_and_absorb_reforms_them(host, binding, pkg):
    D, n = 5, 300
    groups = [[0], [1, 3], [2, 4]]
    rng = np.random.default_rng(3)
    wk = pkg.Worker(pkg.PRIOR_NIW, D, n, device=0, seed=1)
    wk.upload_points(rng.standard_normal((n, D)).astype(np.float32))
    outs = dict(group_mahalanobis=np.empty((n, 3), np.float32), group_tail=np.empty((n, 3), np.float32))
    with pytest.raises(binding.DpmmError, match="dpmm_set_predictive_niw first") as e:
        wk.set_explain_groups(groups, np.zeros(wk.K * 7))                                                # (no clusters yet: W is empty)
    assert e.value.code == -4                                                                            # DPMM_ESTATE
    pars = S.niw_params(rng, D, K)
    wk.set_predictive_niw(*pars)
    with pytest.raises(binding.DpmmError, match="dpmm_set_explain_groups") as e:                         # no tables yet
        wk.explain_groups_points_into(outs)
    assert e.value.code == -4
    cond = importlib.import_module(pkg.__name__ + ".host.condition")
    W = cond.group_factors(pars[1], groups)
    wk.set_explain_groups(groups, W)
    assert wk.explain_groups_points_into(outs) == (0, 0)
    wide = dict(group_mahalanobis=np.full((n, 7), -7.0, np.float32), group_tail=np.full((n, 7), -7.0, np.float32))      # ld > G: the words behind stay
    assert wk.explain_groups_points_into(wide) == (0, 0)
    for name in outs:
        assert same(outs[name], wide[name][:, :3]) and np.all(wide[name][:, 3:] == -7), name
    for bad, why in (([[0, 1], [1, 2]], "two groups"), ([[1, 0]], "increase strictly"), ([[0, D]], "features"), ([[]], "offsets")):
        with pytest.raises(binding.DpmmError, match=why) as e:
            wk.set_explain_groups(bad, np.ones(K * sum(len(g) * (len(g) + 1) // 2 for g in bad)))
        assert e.value.code == -1                                                                        # DPMM_EINVAL
    with pytest.raises(binding.DpmmError, match="W") as e:
        wk.set_explain_groups(groups, np.where(np.arange(W.size) == 5, np.nan, W.ravel()))
    assert e.value.code == -1
    again = {name: np.empty_like(a) for name, a in outs.items()}                                         # a refused call changes nothing: the tables stay in force
    assert wk.explain_groups_points_into(again) == (0, 0) and all(same(outs[name], again[name]) for name in outs)
    wk.set_predictive_niw(*pars)                                                                         # a new parameter set, the tables are the old one's
    with pytest.raises(binding.DpmmError, match="predictive parameters in force") as e:
        wk.explain_groups_points_into(outs)
    assert e.value.code == -4
    wk.close()
    mult = pkg.Worker(pkg.PRIOR_MULT, D, n, device=0, seed=1)
    with pytest.raises(binding.DpmmError, match="NIW") as e:
        mult.set_explain_groups(groups, np.zeros(0))
    assert e.value.code == -1
    mult.close()
    # through the Predictor: absorb re-forms the tables, and the answer is that of the absorbed model
    post, m, A, df = EG.case_model(D, True)
    with open_predictor(host, post, CAP) as p:
        X = drawn_points(p, m, A, groups, 9)
        before = p.explain_groups(X, groups)
        p.absorb(X[:, :200])
        params = worker_params(p)
        got = p.explain_groups(X, groups)
        check(got, p.typicality(X), p.explain(X), X, params, groups, "after absorb")
        assert not same(got.group_mahalanobis, before.group_mahalanobis)


# ------------------------------------------------------------------------------------------------ nothing read that was not written
def test_bits_do_not_depend_on_lds_and_register_contents(host, binding):
    try:
        poison.build()
    except Exception as e:  # noqa: BLE001 -- the tool is test infrastructure
        pytest.skip(f"tests/tools/libpoison.so cannot be built here: {e}")
    D, name, groups = EG.CASES[6]                                                                        # D = 130: three tiles of LDS strip, two row tiles
    post, m, A, df = EG.case_model(D, True)
    out = []
    for dirty in (False, True):
        with open_predictor(host, post, CAP) as p:
            X = drawn_points(p, m, A, groups, 77 + D)
            if dirty:
                with poison.poisoned_kernel_launches(binding, 0xffffffff) as launches:
                    out.append(p.explain_groups(X, groups))
                assert launches[0] > 6, launches
            else:
                out.append(p.explain_groups(X, groups))
    assert same_exp(out[0], out[1]) and not np.isnan(as_np(out[0].group_tail)).any()
