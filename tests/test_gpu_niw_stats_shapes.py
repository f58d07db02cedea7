"""The segmented NIW statistics pass (csrc/suffstats.hip: niw_stats_kernel<NBK>, niw_stats_body / niw_stats_body_shared, niw_reduce_kernel,
launch_niw_row_offsets; the range partition of csrc/stats_ranges.h) against an EXACT reference, at the shapes where it can go wrong.

Exact: the points are integer-valued Float32 (integers in [-1000, 1000] plus a per-feature offset in [-500, 500]); with n < 10 000 every
product and every partial sum is an integer far below 2^53, hence exact in Float64 in ANY order -- through the FP64 matrix instruction,
through the slabs of however many workgroups, through the derived rows `cache - computed`.  The reference is numpy on int64 (per bin N,
sum x, X'X, written into the documented packed layout [0] N, [1..D] sum, [1 + D + a(a+1)/2 + b] S[a][b], a >= b) and every comparison
is an equality: one point dropped, counted twice or taken from a neighbouring bin, one element of one row misplaced, fails it.

Planted, not random, bin populations (COUNTS_SMALL / COUNTS_BIG: 0, 1, 2, 3, 4, 5, ... around the k-step of 4 points, the LDS batch of 16,
the item of 32 / 256 points, and one bin of many items), points in bin order and shuffled; D on both sides of every kernel boundary
(16|17, 32|33, 64|65, 128|129) and of the row padding (61, 62: ldx = 64; 65, 129: the widest pad of a shared-data-path kernel); K around
the lane-64 split of the register-resident bin table and its switch to the global look-up at 128 bins, up to 1024; the partition at
groups = 1 .. 4096 (and beyond the clamp) x items = default, 1, 3; shards of 1 .. 5 points.  Passes: the full pass, the subset pass,
the per-step pass without and with derived rows (a second and third step after a few points moved), each twice for identical bytes.

The one inequality in this file is the summation bound of the real-valued test at the end (derived there, not measured)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, FIRST = 4242, 777
# points per bin; D <= 64: items of 32 points, k-steps of 4; D > 64: items of 256 points, LDS batches of 16
COUNTS_SMALL = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 1500]
COUNTS_BIG = [0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 255, 256, 257, 511, 512, 513, 3000]
ALL_D = [1, 2, 15, 16, 17, 31, 32, 33, 61, 62, 63, 64, 65, 127, 128, 129, 255, 256]
NBK_D = [16, 17, 33, 65, 129]                      # one D of every kernel (NBK = 1, 2, 4, 8, 16)
GROUPS = [0, 1, 2, 3, 7, 4096, 5000]               # 0: the default; 5000 is clamped to NIW_STATS_MAX_GROUPS
ITEMS = [0, 1, 3]                                   # 0: the default (the chunk stays at its minimum); 1: every bin is one item


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


def _counts(D):
    return COUNTS_SMALL if D <= 64 else COUNTS_BIG


_X = {}


def _points(D, n):
    """Integer-valued Float32 points, the same for every test of one (D, n)."""
    if (D, n) not in _X:
        rng = np.random.default_rng(100003 * D + n)
        Xi = rng.integers(-1000, 1001, (n, D)) + rng.integers(-500, 501, D)
        X = Xi.astype(np.float32)
        assert np.array_equal(X.astype(np.int64), Xi)
        _X[(D, n)] = X
    return _X[(D, n)]


def _planted(D, K, order):
    """Labels and sub-labels with the planted bin populations: count j goes to bin round(j (2K - 1) / (L - 1)) -- the first count to the
    first bin, the last one to the last bin, the others spread evenly, so that bins beyond 64 and beyond 128 hold points -- or, when the
    list is longer than the 2K bins, to bin j mod 2K.  Every other bin, and with it most clusters of a large K, stays empty."""
    counts = _counts(D)
    nb, L = 2 * K, len(counts)
    per_bin = np.zeros(nb, np.int64)
    for j, c in enumerate(counts):
        per_bin[(j * (nb - 1) + (L - 1) // 2) // (L - 1) if nb >= L else j % nb] += c
    assert per_bin.sum() == sum(counts) < 10000
    bins = np.repeat(np.arange(nb), per_bin)
    if order == "shuffled":
        bins = np.random.default_rng(7 * D + K).permutation(bins)
    return (bins // 2 + 1).astype(np.int64), (bins % 2 + 1).astype(np.int64)


_BASE = {"key": None, "states": []}


def _accumulate(ref, Xi, bins, sign, D):
    tril = np.tril_indices(D)                       # row-major over a >= b: position a (a + 1) / 2 + b
    for b in np.unique(bins[bins >= 0]):
        Xb = Xi[bins == b]
        ref[b, 0] += sign * len(Xb)
        ref[b, 1:1 + D] += sign * Xb.sum(0)
        ref[b, 1 + D:] += sign * (Xb.T @ Xb)[tril]


def _reference(D, X, K, lab, sub):
    """int64 packed rows [2K][1 + D + D (D + 1) / 2] of the labels given (points with a label outside 1..K belong to no bin).  numpy's
    int64 product is slow at D = 256, so a labelling that differs from an earlier one of the same (D, n, K) in a few points is formed from
    that one's rows by taking those points out of their old bins and adding them to their new ones -- integer arithmetic, exact either way."""
    bins = np.where((lab >= 1) & (lab <= K), 2 * (lab - 1) + (sub - 1), -1)
    key = (D, len(X), K)
    if _BASE["key"] != key:
        _BASE["key"], _BASE["states"] = key, []
    Xi = X.astype(np.int64)
    ref = None
    for obins, oref in _BASE["states"]:
        ch = np.flatnonzero(obins != bins)
        if len(ch) == 0:
            return oref
        if len(ch) <= len(X) // 8:
            ref = oref.copy()
            _accumulate(ref, Xi[ch], obins[ch], -1, D)
            _accumulate(ref, Xi[ch], bins[ch], +1, D)
            break
    if ref is None:
        ref = np.zeros((2 * K, 1 + D + D * (D + 1) // 2), np.int64)
        _accumulate(ref, Xi, bins, +1, D)
    assert np.array_equal(ref[:, 0], np.bincount(bins[bins >= 0], minlength=2 * K))
    # the premise of exactness, for the rows and for the cluster rows left + right
    assert 2 * int(np.abs(ref).max(initial=0)) < 2 ** 53
    _BASE["states"] = [(bins, ref)] + _BASE["states"][:5]
    return ref


def _unpacked(ref, K, D):
    """The reference in the form of Worker.unpack: N (K, 3), sum (K, 3, D), S (K, 3, D, D); index 0 the cluster, 1 left, 2 right."""
    l, r = ref[0::2], ref[1::2]
    N = np.stack([l[:, 0] + r[:, 0], l[:, 0], r[:, 0]], 1)
    s = np.stack([l[:, 1:1 + D] + r[:, 1:1 + D], l[:, 1:1 + D], r[:, 1:1 + D]], 1)
    a, b = np.tril_indices(D)
    S = np.zeros((K, 3, D, D), np.int64)
    for j, t in enumerate((l[:, 1 + D:] + r[:, 1 + D:], l[:, 1 + D:], r[:, 1 + D:])):
        S[:, j, a, b] = t
        S[:, j, b, a] = t
    return N, s, S


def _same(got, ref, tag):
    assert got.dtype == np.float64 and got.shape == ref.shape, tag
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        b, e = bad[0]
        raise AssertionError(f"{tag}: {len(bad)} elements differ, first at bin {b} element {e}: got {got[b, e]!r}, exact {ref[b, e]}; "
                             f"rows {sorted(set(bad[:, 0].tolist()))[:12]}")


def _flags(lab, sub, K):
    cnt = np.zeros((K, 2), np.int64)
    inr = (lab >= 1) & (lab <= K)
    np.add.at(cnt, (lab[inr] - 1, sub[inr] - 1), 1)
    return ((cnt[:, 0] == 0) | (cnt[:, 1] == 0)).astype(np.uint8)


def _step(wk, X, K, lab, sub, epoch, tag):
    """One per-step pass on the labels given, and the same pass again: flags = "a sub-cluster was empty before the reset", labels kept,
    sub-labels changed in flagged clusters only, rows = the exact rows of the labels read back.  Returns those labels."""
    D = X.shape[1]
    wk.set_labels(lab, sub)
    rows, bad = wk.step_stats(epoch)
    glab, gsub = wk.get_labels()
    want_bad = _flags(lab, sub, K)
    assert np.array_equal(bad, want_bad), tag
    assert np.array_equal(glab, lab), tag
    inr = (lab >= 1) & (lab <= K)
    kept = np.ones(len(lab), bool)
    kept[inr] = want_bad[lab[inr] - 1] == 0
    assert np.array_equal(gsub[kept], sub[kept]) and set(np.unique(gsub)) <= {1, 2}, tag
    _same(rows, _reference(D, X, K, glab, gsub), tag)
    # the same epoch again: a cluster that is still one-sided gets the same draw, so labels and bytes repeat (derive: now from the cache)
    rows2, _ = wk.step_stats(epoch)
    l2, s2 = wk.get_labels()
    assert np.array_equal(l2, glab) and np.array_equal(s2, gsub), tag + " (again)"
    assert rows2.tobytes() == rows.tobytes(), tag + " (again)"
    return glab, gsub


def _battery(wk, binding, X, K, lab, sub, tag, unpack=True):
    """Every pass of the statistics on one labelling."""
    n, D = X.shape
    wk.set_labels(lab, sub)
    ref = _reference(D, X, K, lab, sub)
    # the full pass
    full = wk.suffstats_packed()
    _same(full, ref, tag + " full")
    assert wk.suffstats_packed().tobytes() == full.tobytes(), tag + " full (again)"
    if unpack:
        for g, w, name in zip(wk.unpack(full), _unpacked(ref, K, D), ("N", "sum", "S")):
            assert np.array_equal(g, w), f"{tag} unpack {name}"
    # the subset pass: unselected rows are exactly zero
    idx = sorted({K, 1, (K + 1) // 2})
    part = wk.suffstats_packed(idx)
    want = np.zeros_like(ref)
    for k in idx:
        want[2 * k - 2:2 * k] = ref[2 * k - 2:2 * k]
    _same(part, want, tag + f" subset {idx}")
    assert wk.suffstats_packed(idx).tobytes() == part.tobytes(), tag + " subset (again)"
    # the per-step pass, every row computed
    wk.set_option(binding.OPT_STATS_DERIVE, 0)
    _step(wk, X, K, lab, sub, 11, tag + " step derive=0")
    # ... and with derived rows: a first step fills the cache, then five points change cluster -- one of them to a label out of range --
    # and one sub-label flips; then the point comes back.  Rows are a mix of computed rows and cache - computed.
    wk.set_option(binding.OPT_STATS_DERIVE, 1)
    glab, gsub = _step(wk, X, K, lab, sub, 11, tag + " step derive=1")
    rng = np.random.default_rng(n + 31 * K + D)
    moved = rng.choice(n, min(n, 5), replace=False)
    lab2, sub2 = glab.copy(), gsub.copy()
    lab2[moved] = rng.integers(1, K + 1, len(moved))
    lab2[moved[0]] = K + 1
    sub2[moved[-1]] = 3 - sub2[moved[-1]]
    lab2, sub2 = _step(wk, X, K, lab2, sub2, 12, tag + " second step")
    lab3 = lab2.copy()
    lab3[moved[0]] = glab[moved[0]]
    _step(wk, X, K, lab3, sub2, 13, tag + " third step")


def _worker(pkg, X, items=0):
    from dpmmsubclusters_jl_amd import binding
    n, D = X.shape
    wk = pkg.Worker(pkg.PRIOR_NIW, D, n, first_index=FIRST, device=0, seed=SEED)
    wk.upload_points(X)
    if items:
        wk.set_option(binding.OPT_STATS_ITEMS, items)          # (before the first K)
    return wk, binding


@pytest.mark.parametrize("D", ALL_D)
def test_every_dimension(pkg, D):
    K = 11
    X = _points(D, sum(_counts(D)))
    wk, binding = _worker(pkg, X)
    wk.set_num_clusters(K)
    for order in ("sorted", "shuffled"):
        lab, sub = _planted(D, K, order)
        assert _flags(lab, sub, K).any()                      # a one-sided cluster: the bad-cluster reset runs
        _battery(wk, binding, X, K, lab, sub, f"D={D} K={K} {order}")
    wk.close()


@pytest.mark.parametrize("D,K", [(D, K) for K in (1, 31, 32, 33, 63, 64, 65) for D in NBK_D] + [(17, 300), (65, 300), (17, 1024)])
def test_cluster_counts(pkg, D, K):
    """K around the lane-64 split of the register-resident bin table (2K = 62 .. 130 bins) and its switch to find_bin at 128 bins."""
    X = _points(D, sum(_counts(D)))
    wk, binding = _worker(pkg, X)
    wk.set_num_clusters(K)
    for order in ("sorted", "shuffled"):
        lab, sub = _planted(D, K, order)
        _battery(wk, binding, X, K, lab, sub, f"D={D} K={K} {order}")
    wk.close()


@pytest.mark.parametrize("items", ITEMS)
@pytest.mark.parametrize("D", [16, 64, 65, 256])
def test_partition_options(pkg, D, items):
    """groups = 1: every head but one lives in slot NIW_STATS_MAX_GROUPS + bin; groups >= items: every item is a workgroup boundary."""
    K = 11
    X = _points(D, sum(_counts(D)))
    wk, binding = _worker(pkg, X, items)
    wk.set_num_clusters(K)
    for order in ("sorted", "shuffled"):
        lab, sub = _planted(D, K, order)
        for groups in GROUPS:
            wk.set_option(binding.OPT_STATS_GROUPS, groups)
            _battery(wk, binding, X, K, lab, sub, f"D={D} items={items} groups={groups} {order}", unpack=False)
    wk.close()


@pytest.mark.parametrize("D", [16, 64, 65, 256])
def test_tiny_shards(pkg, D):
    """1 .. 5 points: one cluster, and more bins than points."""
    for n in (1, 2, 3, 5):
        X = _points(D, n)
        wk, binding = _worker(pkg, X)
        rng = np.random.default_rng(n + D)
        for K in (1, 33):
            wk.set_num_clusters(K)
            for rep in range(2):                                # all in the last bin; scattered
                lab = np.full(n, K, np.int64) if rep == 0 else rng.integers(1, K + 1, n).astype(np.int64)
                sub = np.full(n, 2, np.int64) if rep == 0 else rng.integers(1, 3, n).astype(np.int64)
                _battery(wk, binding, X, K, lab, sub, f"D={D} n={n} K={K} rep={rep}")
        wk.close()


@pytest.mark.parametrize("D", NBK_D)
def test_packed_layout_element_by_element(pkg, D):
    """Every element of two raw packed rows recomputed from the documented layout, one index at a time: the integer data make the S[a][b]
    of a row distinct (but for a chance pair), so a transposed or misplaced element of row_off / inv_off cannot hide behind an equal value."""
    K = 11
    X = _points(D, sum(_counts(D)))
    wk, _ = _worker(pkg, X)
    wk.set_num_clusters(K)
    lab, sub = _planted(D, K, "shuffled")
    wk.set_labels(lab, sub)
    rows = wk.suffstats_packed()
    assert rows.shape == (2 * K, 1 + D + D * (D + 1) // 2)
    Xi = X.astype(np.int64)
    for b in (2 * K - 1, 2 * K - 2):                           # the largest bin and its neighbour
        Xb = Xi[(2 * (lab - 1) + (sub - 1)) == b]
        assert len(Xb) > D
        row = rows[b]
        assert row[0] == len(Xb)
        for a in range(D):
            assert row[1 + a] == int(Xb[:, a].sum()), (b, a)
        S = Xb.T @ Xb
        assert len(set(S[np.tril_indices(D)].tolist())) >= D * (D + 1) // 2 - 2      # distinct (one pair of 8385 coincides at D = 129)
        for a in range(D):
            for c in range(a + 1):
                assert row[1 + D + a * (a + 1) // 2 + c] == int(S[a, c]), (b, a, c)
    wk.close()


@pytest.mark.parametrize("D", [17, 64, 65, 129, 256])
def test_real_valued_accuracy(pkg, D):
    """Gaussian Float32 data, mean 1e3 and sd 1 (the worst case for a one-pass scatter sum), against np.longdouble accumulation.  The
    bound is the standard one of a recursive sum in any order: a product of two Float32 values is exact in Float64, so only the additions
    round, at most cnt - 1 of them on the way of any term, each by 2^-53 relative:
        |S_ab - exact| <= cnt 2^-52 sum_i |x_ia x_ib|,    |s_a - exact| <= cnt 2^-52 sum_i |x_ia|
    (the data are positive, so the sums of absolute values are the exact sums themselves)."""
    K, per_bin = 3, [1, 5, 17, 64, 300, 1200]                  # (np.longdouble products are slow: a shorter list of planted counts)
    n = sum(per_bin)
    X = (1e3 + np.random.default_rng(D).normal(size=(n, D))).astype(np.float32)
    assert (X > 0).all()
    wk, _ = _worker(pkg, X)
    wk.set_num_clusters(K)
    bins = np.random.default_rng(D + 1).permutation(np.repeat(np.arange(2 * K), per_bin))
    wk.set_labels((bins // 2 + 1).astype(np.int64), (bins % 2 + 1).astype(np.int64))
    Xl = X.astype(np.longdouble)
    tril = np.tril_indices(D)
    ref = np.zeros((2 * K, 1 + D + D * (D + 1) // 2), np.longdouble)
    for b in np.unique(bins):
        Xb = Xl[bins == b]
        ref[b, 0] = len(Xb)
        ref[b, 1:1 + D] = Xb.sum(0)
        ref[b, 1 + D:] = (Xb.T @ Xb)[tril]
    bound = ref[:, :1] * np.longdouble(2.0) ** -52 * ref
    rows = wk.suffstats_packed()
    assert np.array_equal(rows[:, 0], ref[:, 0].astype(np.float64))
    err = np.abs(rows.astype(np.longdouble) - ref)[:, 1:]
    bound = bound[:, 1:]
    worst = float((err / np.maximum(bound, np.longdouble(1e-300))).max())
    print(f"D={D}: largest |error| / bound = {worst:.3g}")
    assert np.all(err <= bound), worst
    wk.close()
