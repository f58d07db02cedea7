"""tests/tools/niw_routes.py without a GPU: the launcher's LDS thresholds (whoever changes launch_direct's budget has to move the cases of
tests/test_gpu_niw_routes.py with it), the separation of paired_problem's sites for every case of that module, and the evaluated set the
helper predicts for the two compact-table cases."""
import numpy as np
import pytest

from oracle import oracle as orc
from test_gpu_niw import table_f64 as table_f64_oracle
from tools import niw_routes as nr


def test_budgets_restates_launch_direct():
    assert nr.budgets(1) == dict(rows=39, compact_slots=19, screen_lds_max=None)
    assert nr.budgets(2) == dict(rows=52, compact_slots=26, screen_lds_max=25)
    assert nr.budgets(4) == dict(rows=79, compact_slots=39, screen_lds_max=38)
    assert [nr.nb_of(D) for D in (1, 16, 17, 32, 33, 64, 65, 128, 129, 256)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert [nr.screen_block(D) for D in (3, 17, 32, 33, 36, 48, 49, 64, 72, 128, 132, 256)] == [0, 1, 1, 2, 2, 2, 3, 3, 4, 7, 8, 15]


def test_cases_sit_on_the_thresholds():
    """Every threshold of budgets() has a case at it, one below or above it, for the smallest and the largest D of its kernel."""
    have = {(D, K) for D, K, v in nr.all_cases() if v == "sorted"}
    for D in (3, 16):
        assert {(D, K) for K in (39, 40, 41)} <= have
    for D in (17, 32):
        b = nr.budgets(2)
        assert {(D, K) for K in (b["screen_lds_max"], b["screen_lds_max"] + 1, b["rows"], b["rows"] + 1)} <= have
    for D in (33, 64):
        b = nr.budgets(4)
        assert {(D, K) for K in (b["screen_lds_max"], b["screen_lds_max"] + 1, b["rows"], b["rows"] + 1)} <= have


def test_table_f64_is_the_oracles():
    """The helper's numpy table is the oracle's Float64 evaluation (which carries the reference's -D^2/2 log 2 pi, mv_gaussian.jl:24)."""
    P = nr.paired_problem(20, 300, 7, seed=3)
    want = table_f64_oracle(P) + 0.5 * 20 * 20 * np.log(2 * np.pi)
    np.testing.assert_allclose(nr.table_f64(P), want, rtol=1e-12, atol=1e-9)
    # the 16-row bound is an upper bound of the value, and the whole value when the rows start at 0
    assert np.all(nr.table_f64(P, screen_rows_from=16) >= nr.table_f64(P) - 1e-9)
    np.testing.assert_allclose(nr.table_f64(P, screen_rows_from=0), nr.table_f64(P), rtol=1e-10, atol=1e-8)
    olab = orc.sample_log_cat(nr.table_f64(P).astype(np.float32), np.full(300, 0.5, np.float32))
    assert olab.min() >= 1 and olab.max() <= 7


@pytest.mark.parametrize("D,K,variant", nr.all_cases())
def test_sites_are_separated(D, K, variant):
    """Under any cluster of another site a point's probability is below 2^-149 of its row maximum (an exact zero of the Float32 draw) and
    below the screens' margin with 50 nats to spare; the partner at the same site keeps visible mass for most points."""
    P = nr.case_problem(D, K, variant)
    T = nr.table_f64(P)
    sep = nr.separation(P, T)
    assert sep < -nr.LOG_DENORMAL - nr.MARGIN, sep
    S = P["S"]
    partner = np.where(P["z"] < S, P["z"] + S, P["z"] - S)
    has = partner < K
    i = np.flatnonzero(has)
    rel = T[partner[i], i] - T.max(0)[i]
    assert np.median(rel) > -10.0 and rel.min() > -nr.MARGIN + 10.0, (np.median(rel), rel.min())
    assert len(np.unique(P["z"])) == (K if variant != "boundary" else K - 32)
    if variant == "boundary":
        assert 31 in P["z"] and 64 in P["z"] and not np.isin(P["z"], np.arange(32, 64)).any()
    if variant == "wrong":
        r = nr.rotated_labels(P)
        assert r.min() >= 0 and r.max() < K and np.all(P["site"][r] != P["site"][P["z"]])


def _nev(D, K, variant):
    P = nr.case_problem(D, K, variant)
    T = nr.table_f64(P)
    U = nr.table_f64(P, screen_rows_from=16 * nr.screen_block(D))
    sub = 1 + (np.arange(P["n"]) & 1)
    order = nr.visiting_order(P["z"], sub) if variant == "sorted" else np.arange(P["n"])
    sets = nr.tile_sets(P, T, U, order, P["z"], extra_refs=2)
    return P, sets


@pytest.mark.parametrize("D", [17, 32])
def test_compact_slots_predicted(D):
    """K = 129 > 52 rows: the generic kernel with 26 compact slots.  (a) sorted: every tile's evaluated set is known and fits the slots.
    (b) mixed: it is known as well, exceeds the slots in most tiles and fills them exactly in some."""
    slots = nr.budgets(2)["compact_slots"]
    P, sets = _nev(D, 129, "sorted")
    assert all(sure == may for _, sure, may in sets)
    nev = np.array([len(s) for _, s, _ in sets])
    blocks = (64 - 2) // (P["n"] // 129) + 2                    # blocks of 23 points a 64-point tile can touch: 4, two clusters per site
    assert nev.max() <= 2 * blocks < slots and nev.min() >= 2
    P, sets = _nev(D, 129, "mixed")
    assert all(sure == may for _, sure, may in sets)
    nev = np.array([len(s) for _, s, _ in sets])
    want = np.array([2 * nr.MIXED_SITES[t % len(nr.MIXED_SITES)] for t in range(len(sets))])
    assert np.all((nev == want) | (nev == want - 1))            # (- 1: the tile holds the site of the one cluster without a partner)
    assert (nev > slots).mean() > 0.5 and (nev == slots).sum() >= 1 and (nev == slots + 1).sum() + (nev == slots + 2).sum() >= 1
