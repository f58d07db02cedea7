"""The inputs of the value-level tests of the Multinomial device master, in one place: tests/test_gpu_mult_master.py feeds them to the
device, tests/test_mult_master_ref_cpu.py checks on the CPU that the reference is well conditioned on every one of them (margin, headroom
of tests/tools/mult_master_ref.py) and that every mutant of the reference is told apart on one of them.  numpy only.

Rows.  Cluster k < 5 of row set v is of kind KINDS[(v + k) % 5], clusters beyond are populated; a case of fewer than five clusters has
five row sets, so that every case meets, at every cluster position: a populated cluster, a one-sided one (right empty), an empty one,
counts up to 1e7 per feature (their Float32 image rounds once left and right are pooled), and rows with a single non-zero feature.
Seeds.  The inputs of a case come from seed 0 unless SEEDS names another: the first seed at which margin >= 1e-8 and headroom >= 256
held for every row set.  test_mult_master_ref_cpu.py asserts the conditions the GPU comparison rests on (1e-9 and 64) on every case."""
import numpy as np

REGIMES = ("tiny", "mixed", "ones", "large")
KINDS = (("big", "single"), ("small", "empty"), ("empty", "empty"), ("single", "small"), ("small", "small"))
MARGIN_MIN, HEADROOM_MIN = 1e-9, 64.0
MAXD, MAXPAIRS = 16384, 8192

DRAW_SHAPES = tuple((D, 2) for D in (1, 2, 255, 256, 257, 1000, 16384)) + tuple((300, K) for K in (1, 64, 1024))
MARGINAL_SHAPES = tuple((D, r) for D in (1, 2, 255, 256, 257, 1000) for r in REGIMES) + ((16384, "large"),)
MARGINAL_K = 8
OUTLIER_FACTOR = 50.0
AHEAD_DIMS = (255, 1000)

# (D, K, regime, outlier) -> seed; outlier: None (no outlier prior), "first" (outlier_first), "unused" (an outlier prior nobody follows)
SEEDS = {(2, 2, "tiny", None): 2}


def alpha_of(D, regime, rng):
    if regime == "tiny":
        return np.full(D, 1e-3, np.float32)
    if regime == "mixed":
        return rng.uniform(0.15, 2.5, D).astype(np.float32)
    if regime == "ones":
        return np.ones(D, np.float32)
    if regime == "large":
        return rng.uniform(1.0, 1e6, D).astype(np.float32)
    raise ValueError(regime)


def _side(kind, D, rng):
    row = np.zeros(1 + D)
    if kind == "small":
        row[1:] = rng.integers(0, 8, D) * (rng.random(D) < 0.7)
        row[1 + rng.integers(0, D)] += 3
        row[1 + rng.integers(0, D)] += 5
        row[0] = rng.integers(1, 50)
    elif kind == "big":
        row[1:] = rng.integers(0, 10_000_001, D)
        row[1 + rng.integers(0, D)] = 1e7
        row[0] = 100_000
    elif kind == "single":
        row[1 + rng.integers(0, D)] = row[0] = rng.integers(1, 20)
    elif kind != "empty":
        raise ValueError(kind)
    return row


def row_sets(K):
    """how many row sets a case of K clusters takes: below five clusters, five -- every cluster position meets every kind"""
    return 5 if K < 5 else 1


def rows_of(D, K, v, rng):
    """rows [2K, 1 + D] Float64 of row set v"""
    out = np.empty((2 * K, 1 + D))
    for k in range(K):
        kind = KINDS[(v + k) % 5] if k < 5 else (("small", "small"), ("big", "small"))[k % 2]
        out[2 * k], out[2 * k + 1] = _side(kind[0], D, rng), _side(kind[1], D, rng)
    return out


class Case:
    """One (D, K, alpha regime, outlier mode): alpha, alpha_outlier, the library seed, the epoch and the row sets."""

    def __init__(self, D, K, regime, outlier=None, seed=None):
        self.D, self.K, self.regime, self.outlier = D, K, regime, outlier
        self.key = (D, K, regime, outlier)
        self.input_seed = SEEDS.get(self.key, 0) if seed is None else seed
        rng = np.random.default_rng([self.input_seed, D, K, REGIMES.index(regime), 0 if outlier is None else 1])
        self.alpha = alpha_of(D, regime, rng)
        self.alpha_outlier = None if outlier is None else (self.alpha * np.float32(OUTLIER_FACTOR)).astype(np.float32)
        self.outlier_first = outlier == "first"
        self.seed = 1000 + 17 * self.input_seed + D
        self.epoch = 3 + self.input_seed % 5
        self.rows = [rows_of(D, K, v, rng) for v in range(row_sets(K))]

    def __repr__(self):
        return "D%d-K%d-%s%s" % (self.D, self.K, self.regime, "" if self.outlier is None else "-outlier_" + self.outlier)


def draw_cases():
    out = [Case(D, K, r) for D, K in DRAW_SHAPES for r in REGIMES]
    return out + [Case(300, 4, r, o) for r in ("mixed", "ones") for o in ("first", "unused")]


def marginal_cases():
    """Cases of MARGINAL_K clusters with an outlier prior set up; each is evaluated with outlier_first off and on."""
    return [Case(D, MARGINAL_K, r, "first") for D, r in MARGINAL_SHAPES]


def all_pairs(K):
    """every ordered pair, i = j included: all C(K, 2), (0, j), (j, 0) and (i, i)"""
    return np.array([(i, j) for i in range(K) for j in range(K)], np.int32)


class AheadCase:
    """Draws launched ahead: byte data of n points in K clusters with both sides populated; rows: the statistics of those labels."""
    n, K = 1500, 3

    def __init__(self, D):
        self.D = D
        self.input_seed = SEEDS.get((D, self.K, "ahead", "first"), 0)
        rng = np.random.default_rng([self.input_seed, D, 77])
        self.X = rng.poisson(0.4, (self.n, D)).astype(np.float32)
        self.labels = 1 + np.arange(self.n) % self.K
        self.sub = 1 + (np.arange(self.n) // self.K) % 2
        self.alpha = rng.uniform(0.15, 2.5, D).astype(np.float32)
        self.alpha_outlier = (self.alpha * np.float32(OUTLIER_FACTOR)).astype(np.float32)
        self.seed = 500 + self.input_seed
        self.epoch0 = 11
        self.rows = np.zeros((2 * self.K, 1 + D))
        np.add.at(self.rows, 2 * (self.labels - 1) + (self.sub - 1), np.concatenate([np.ones((self.n, 1)), self.X.astype(np.float64)], axis=1))
        # (epoch, outlier_first) of every draw compared by value: the set made ahead (the guess: the epoch after the last draw, the flag of the
        # pairs asked for) | another epoch than the guess epoch0 + 2 | the guessed epoch with the other outlier flag
        self.draws = ((self.epoch0 + 1, False), (self.epoch0 + 7, False), (self.epoch0 + 8, True))

    def __repr__(self):
        return "ahead-D%d" % self.D
