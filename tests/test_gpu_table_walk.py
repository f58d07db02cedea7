"""GPU tests of the walk over the score table that every call of the predictor headers makes (csrc/dpmm_api.cpp: walk_open, walk_ranges,
the staging of the host variants' outputs, the session record and the counter fold of the accumulators).

Two workers at the smallest shape that has whole tiles, a ragged end and a choice of ranges -- n = 3 tiles + 5 points, K = 3: an NIW one
(D = 4, DPMM_OPT_SCORE_MISSING on; in the first tile two points carry a NaN feature and one +Inf) and a Multinomial one (D = 8, Float32
store).  Two table budgets: A, the default, holds all of n in one range; B = rstep K tile sizeof(float) bytes holds exactly one tile, so a
call walks four ranges, the last of 5 points.

  per-point calls   score_points (all five outputs, m = 2), typicality_points, impute_points, impute_draw_points (2 draws, components): the
                    host and the device variant under A and under B write the same bits and report the same counters.
  accumulators      rank, overlap, batchstats (hard / soft, with and without min_tail), countstats (hard) over n_valid = one tile + 7
                    points: under B -- two ranges, 7 points of the second -- the integer counters equal those under A; rank's lists and
                    hard countstats are exact, so all of their outputs do.  The Float64 sums of overlap and batchstats are held, under
                    either budget, to the numpy references of tests/tools at the bounds of tests/test_gpu_overlap.py (relative n 2^-52) and
                    tests/test_gpu_batchstats.py (2 gamma(n + 2) T), from the labels, probabilities and tails the same worker returns."""
import importlib

import numpy as np
import pytest
import torch

import test_gpu_score as S
from tools import batchstats_ref as B
from tools import overlap_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = 3
TILE = 256
N = 3 * TILE + 5
N_VALID = TILE + 7
GAPS, LOST = [3, 100], [200]          # points of the first tile with a NaN feature | with +Inf
MIN_TAIL = 0.25


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def binding(pkg):
    return importlib.import_module(pkg.__name__ + ".binding")


def budget_b(kind):
    """MB of one tile of the table, as score_table_slab counts: rstep * K rows of `tile` floats."""
    return (1 if kind == "niw" else 3) * K * TILE * 4 / 2.0 ** 20


def niw_worker(pkg, binding):
    D = 4
    assert S.tile_of("niw", D) == TILE
    rng = np.random.default_rng(2024)
    par = S.niw_params(rng, D, K)
    X = S.niw_points(rng, D, N, par[0])
    X[GAPS[0], 1] = np.nan
    X[GAPS[1], 3] = np.nan
    X[LOST[0], 0] = np.inf
    wk = pkg.Worker(pkg.PRIOR_NIW, D, N, device=0, seed=1)
    wk.upload_points(X)
    wk.set_predictive_niw(*par)
    wk.set_option(binding.OPT_SCORE_MISSING, 1)
    return wk, X


def mult_worker(pkg):
    D = 8
    assert S.tile_of("mult", D) == TILE
    rng = np.random.default_rng(2025)
    X = rng.poisson(0.8, (N, D)).astype(np.float32)
    X += np.float32(0.3) * (rng.random((N, D)) < 0.3)                  # 0.3 is not a bf16 value: the Float32 store
    wk = pkg.Worker(pkg.PRIOR_MULT, D, N, device=0, seed=1)
    wk.upload_points(X)
    wk.set_predictive_mult(*S.mult_params(rng, D, K))
    return wk, X


@pytest.fixture(scope="module")
def niw(pkg, binding):
    wk, X = niw_worker(pkg, binding)
    yield wk, X
    wk.close()


@pytest.fixture(scope="module")
def mult(pkg):
    wk, X = mult_worker(pkg)
    yield wk, X
    wk.close()


def as_np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def same(a, b):
    """Equal shapes, types and bits."""
    a, b = np.ascontiguousarray(as_np(a)), np.ascontiguousarray(as_np(b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def empty(shape, dtype, device):
    return torch.empty(shape, dtype=getattr(torch, dtype), device=DEV) if device else np.empty(shape, dtype)


# ------------------------------------------------------------------------------------------------ the calls: {name: array} each
def score(wk, device):
    out = wk.score_points(labels=True, logdens=True, m=2, probs=True, device=DEV if device else None)
    out["missing_counts"] = np.array(wk.score_missing_counts())
    return out


def typicality(wk, device):
    out = dict(labels=empty(wk.n, "int64", device), mahalanobis=empty(wk.n, "float32", device), tail=empty(wk.n, "float32", device))
    out["skipped_incomplete"] = np.array(wk.typicality_points_into(out))
    out["missing_counts"] = np.array(wk.score_missing_counts())
    return out


def impute(wk, device):
    out = dict(rows=empty((wk.n, wk.D + 3), "float32", device))       # ld > D: the padding of the host variant's rows is written too
    wk.impute_points_into(out["rows"])
    out["missing_counts"] = np.array(wk.score_missing_counts())
    return out


def impute_draws(wk, device):
    out = dict(draws=empty((wk.n, 2, wk.D), "float32", device), comp=empty((2, wk.n), "int32", device))
    wk.impute_draws_into(out["draws"], seed=77, i0=1000, draw0=1, comp=out["comp"])
    out["missing_counts"] = np.array(wk.score_missing_counts())
    return out


def rank(wk, device=False):
    wk.rank_begin(4)
    wk.rank_accumulate(5000, N_VALID)
    return wk.rank_read(device=DEV if device else None)


def overlap(wk, device=False):
    wk.overlap_begin()
    wk.overlap_accumulate(N_VALID)
    return wk.overlap_read()


def batchstats(mode, min_tail):
    def call(wk, device=False):
        wk.batchstats_begin(mode)
        wk.batchstats_set_min_tail(min_tail)
        wk.batchstats_accumulate(N_VALID)
        return wk.batchstats_read()
    return call


def countstats(wk, device=False):
    wk.countstats_begin(0)
    wk.countstats_accumulate(N_VALID)
    return wk.countstats_read()


def under(wk, binding, kind, budget, call, device=False):
    """The outputs of `call` under budget "A" or "B"."""
    wk.set_option(binding.OPT_SCORE_TABLE_MB, -1 if budget == "A" else budget_b(kind))
    try:
        return {k: as_np(v) for k, v in call(wk, device).items()}
    finally:
        wk.set_option(binding.OPT_SCORE_TABLE_MB, -1)


# ------------------------------------------------------------------------------------------------ per-point calls
@pytest.mark.parametrize("kind,call", [("niw", score), ("mult", score), ("niw", typicality), ("niw", impute), ("niw", impute_draws)],
                         ids=["score-niw", "score-mult", "typicality", "impute", "impute_draws"])
def test_host_and_device_variants_under_both_budgets_write_the_same_bits(binding, niw, mult, kind, call):
    wk, X = niw if kind == "niw" else mult
    base = under(wk, binding, kind, "A", call)
    for budget, device in (("A", True), ("B", False), ("B", True)):
        got = under(wk, binding, kind, budget, call, device)
        assert got.keys() == base.keys()
        for k in base:
            assert same(got[k], base[k]), (call.__name__, budget, "device" if device else "host", k)
    if kind == "niw":                                                  # the walk ran the missing-feature pass on every range, once
        assert tuple(base["missing_counts"]) == (len(GAPS), 0)
    else:
        assert tuple(base["missing_counts"]) == (0, 0)
    if call is typicality:
        assert tuple(base["skipped_incomplete"]) == (len(LOST), len(GAPS)) and np.isnan(base["tail"][GAPS + LOST]).all()
    if call is impute:
        gap = np.isnan(X)
        assert same(base["rows"][:, :wk.D][~gap], X[~gap]) and np.isfinite(base["rows"][:, :wk.D][gap]).all() and not base["rows"][:, wk.D:].any()
    if call is impute_draws:
        assert (base["comp"][:, GAPS] >= 0).all() and (np.delete(base["comp"], GAPS, axis=1) == -1).all()
        assert not same(base["draws"][GAPS, 0], base["draws"][GAPS, 1])


# ------------------------------------------------------------------------------------------------ accumulators over n_valid = one tile + 7
def test_rank_lists_and_counters_do_not_depend_on_the_ranges(binding, niw, mult):
    for kind, (wk, _) in (("niw", niw), ("mult", mult)):
        base = under(wk, binding, kind, "A", rank)
        assert int(base["skipped"][0]) == (len(LOST) if kind == "niw" else 0) and int(base["count"].sum()) + int(base["skipped"][0]) == N_VALID
        for idx in (base["typ_idx"], base["fringe_idx"]):              # nothing beyond n_valid is ranked
            assert (idx >= 0).any() and np.all((idx == -1) | ((idx >= 5000) & (idx < 5000 + N_VALID)))
        for budget, device in (("A", True), ("B", False), ("B", True)):
            got = under(wk, binding, kind, budget, rank, device)
            for k in base:
                assert same(got[k], base[k]), (kind, budget, device, k)


def test_hard_countstats_do_not_depend_on_the_ranges(binding, mult):
    wk, X = mult
    base = under(wk, binding, "mult", "A", countstats)
    got = under(wk, binding, "mult", "B", countstats)
    for k in base:
        assert same(got[k], base[k]), k
    assert int(base["count"].sum()) == N_VALID and base["skipped"][0] == base["held_out"][0] == base["incomplete"][0] == 0
    assert np.array_equal(base["N"], base["count"].astype(np.float64))
    assert np.abs(base["sums"].sum(0) - X[:N_VALID].astype(np.float64).sum(0)).max() <= N_VALID * 2.0 ** -52 * X[:N_VALID].sum(0).max()


@pytest.fixture(scope="module")
def scored(binding, niw):
    """Labels, probabilities, log-densities and tails of the NIW worker's points under budget A: what the references are made from."""
    wk, X = niw
    s = under(wk, binding, "niw", "A", score)
    t = under(wk, binding, "niw", "A", typicality)
    return dict(labels=s["labels"], probs=s["probs"], logdens=s["logdens"], tail=t["tail"])


def test_overlap_counters_and_sums_over_two_ranges(binding, niw, scored):
    wk, _ = niw
    nv = N_VALID
    want = overlap_ref.from_probs(scored["probs"][:nv], scored["labels"][:nv])
    assert want["skipped"] == len(LOST)
    a, b = under(wk, binding, "niw", "A", overlap), under(wk, binding, "niw", "B", overlap)
    for got in (a, b):
        assert np.array_equal(got["count"], want["count"]) and int(got["skipped"][0]) == want["skipped"]
        assert overlap_ref.close(got["overlap"], want["overlap"], nv) and overlap_ref.close(got["mass"], want["mass"], nv)
    assert same(a["count"], b["count"]) and same(a["skipped"], b["skipped"])


@pytest.mark.parametrize("min_tail", [None, MIN_TAIL], ids=["no_tail", "min_tail"])
@pytest.mark.parametrize("mode", ["hard", "soft"])
def test_batchstats_counters_and_sums_over_two_ranges(binding, niw, scored, mode, min_tail):
    wk, X = niw
    nv = N_VALID
    with np.errstate(invalid="ignore"):
        held = np.zeros(nv, bool) if min_tail is None else scored["tail"][:nv] < np.float32(min_tail)      # (NaN compares false: skipped and incomplete points)
    keep = ~held
    want = B.stats(X[:nv][keep].T, scored["labels"][:nv][keep], scored["probs"][:nv][keep], mode)
    want["held_out"] = int(held.sum())
    assert (want["skipped"], want["incomplete"]) == (len(LOST), len(GAPS)) and (min_tail is None or 20 < want["held_out"] < nv - 20)
    call = batchstats(1 if mode == "soft" else 0, min_tail)
    a, b = under(wk, binding, "niw", "A", call), under(wk, binding, "niw", "B", call)
    for name, got in (("A", a), ("B", b)):
        assert np.array_equal(got["count"], want["count"]), name
        assert (int(got["skipped"][0]), int(got["incomplete"][0]), int(got["held_out"][0])) == (want["skipped"], want["incomplete"], want["held_out"]), name
        w = B.within(got, want, nv)
        print(mode, min_tail, "budget", name, "largest difference in units of the bound 2 gamma(n + 2) T:", w)
        assert w <= 1, (name, w)
    for k in ("count", "skipped", "incomplete", "held_out"):
        assert same(a[k], b[k]), k
