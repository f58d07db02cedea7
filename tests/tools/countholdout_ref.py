"""numpy reference of the class rule of include/dpmm_hip_countholdout.h and of the prefix rule of its caps.

`classes` is the rule on what the library's own `score_samples` returns: a point is skipped when its log-density is not finite, else held
out by the raw floor or by the floor per count, else incomplete when a value of it is not finite, else it takes part.  X is dense (D, n) or
scipy CSC (D, n); for CSC only stored entries count, as the sparse store has it."""
import numpy as np


def totals_and_complete(X):
    """(t (n,) float64, complete (n,) bool): the Float64 total of every point's values and whether all of them are finite."""
    if hasattr(X, "indptr"):
        cp, val = np.asarray(X.indptr, np.int64), np.asarray(X.data, np.float64)
        n = len(cp) - 1
        col = np.repeat(np.arange(n), np.diff(cp))
        bad = np.zeros(n, bool)
        bad[col[~np.isfinite(val)]] = True
        t = np.zeros(n)
        np.add.at(t, col, np.where(np.isfinite(val), val, 0.0))
        return t, ~bad
    X = np.asarray(X, np.float64)
    fin = np.isfinite(X)
    return np.where(fin, X, 0.0).sum(0), fin.all(0)


def classes(ld, X, f=None, fpc=None):
    """dict of bool (n,) arrays skipped, held, incomplete, part from the Float32 log-densities `ld`, the points and the two floors (None:
    not in use).  held = finite(ld) & (ld < f32(f) | (complete & t > 0 & f64(ld) < f64(f32(fpc)) * t))."""
    ld = np.asarray(ld, np.float32)
    t, complete = totals_and_complete(X)
    scored = np.isfinite(ld)
    held = np.zeros(len(ld), bool)
    if f is not None:
        held |= ld < np.float32(f)
    if fpc is not None:
        with np.errstate(invalid="ignore"):
            held |= complete & (t > 0) & (ld.astype(np.float64) < np.float64(np.float32(fpc)) * t)
    held &= scored
    incomplete = scored & ~held & ~complete
    return dict(skipped=~scored, held=held, incomplete=incomplete, part=scored & ~held & ~incomplete, t=t, complete=complete)


def stored_prefix(lengths, cap, entry_cap):
    """(stored, stored_entries): the longest prefix s of the held-out points with s <= cap and colptr[s] <= entry_cap, lengths their entries."""
    cp = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))])
    s = 0
    while s < len(lengths) and s + 1 <= cap and cp[s + 1] <= entry_cap:
        s += 1
    return s, int(cp[s])
