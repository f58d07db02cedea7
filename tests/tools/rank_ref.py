"""The definitions of include/dpmm_hip_rank.h in numpy: from a (K, n) Float32 table to the typical and fringe lists, counts and `skipped`.

  lab_i   1-based argmax by Julia's rule (the first NaN wins, else the first maximum)
  s_i     max_k table[k][i], NaN skipped
  a point takes part iff its row holds no NaN and s_i is finite; the others are counted in `skipped`
  typical[k]   the first m points with lab == k + 1 that take part by (s descending, index ascending)
  fringe[k]    the first m of them by (s ascending, index ascending)
Unused slots hold index -1 and score NaN.  The sort is np.lexsort on (index, +-s) per label; between the two (a -0.0 and a +0.0 compare
equal as numbers) the header ranks -0.0 below +0.0, which the sign bit, a key between them, restates."""
import numpy as np


def labels_and_scores(table):
    """(lab (n,) int64 1-based, s (n,) float32, part (n,) bool) of a (K, n) Float32 table."""
    table = np.asarray(table, np.float32)
    K, n = table.shape
    nan = np.isnan(table)
    anynan = nan.any(0)
    with np.errstate(all="ignore"):
        s = np.where(nan, -np.inf, table).max(0).astype(np.float32) if K else np.full(n, -np.inf, np.float32)
        first_max = np.argmax(np.where(nan, -np.inf, table) == s[None, :], axis=0)
    lab = np.where(anynan, np.argmax(nan, axis=0), first_max).astype(np.int64) + 1
    part = ~anynan & np.isfinite(s)
    return lab, s, part


def rank(table, m, index_base=0, n_valid=None):
    """dict(typ_idx, typ_score, fringe_idx, fringe_score (K, m), count (K,), skipped int) of the first n_valid columns of `table`,
    whose global indices are index_base + column."""
    table = np.asarray(table, np.float32)
    K, n = table.shape
    n_valid = n if n_valid is None else int(n_valid)
    table = table[:, :n_valid]
    lab, s, part = labels_and_scores(table)
    idx = np.arange(n_valid, dtype=np.int64) + int(index_base)
    out = dict(typ_idx=np.full((K, m), -1, np.int64), typ_score=np.full((K, m), np.nan, np.float32),
               fringe_idx=np.full((K, m), -1, np.int64), fringe_score=np.full((K, m), np.nan, np.float32),
               count=np.zeros(K, np.int64), skipped=int((~part).sum()))
    for k in range(K):
        sel = np.flatnonzero(part & (lab == k + 1))
        out["count"][k] = sel.size
        sk, ik = s[sel], idx[sel]
        neg = np.signbit(sk) & (sk == 0)                          # -0.0 below +0.0
        for name, order in (("typ", np.lexsort((ik, neg, -sk.astype(np.float64)))), ("fringe", np.lexsort((ik, ~neg, sk.astype(np.float64))))):
            o = order[:m]
            out[name + "_idx"][k, :o.size] = ik[o]
            out[name + "_score"][k, :o.size] = sk[o]
    return out


def merge(results, m):
    """The result for the union of disjoint pieces ranked one by one (each a dict as `rank` returns, ranked with the same m)."""
    K = results[0]["count"].size
    out = dict(typ_idx=np.full((K, m), -1, np.int64), typ_score=np.full((K, m), np.nan, np.float32),
               fringe_idx=np.full((K, m), -1, np.int64), fringe_score=np.full((K, m), np.nan, np.float32),
               count=sum(r["count"] for r in results), skipped=sum(r["skipped"] for r in results))
    for k in range(K):
        for name, sign in (("typ", -1.0), ("fringe", 1.0)):
            ik = np.concatenate([r[name + "_idx"][k] for r in results])
            sk = np.concatenate([r[name + "_score"][k] for r in results])
            keep = ik >= 0
            ik, sk = ik[keep], sk[keep]
            neg = np.signbit(sk) & (sk == 0)
            o = np.lexsort((ik, neg if sign < 0 else ~neg, sign * sk.astype(np.float64)))[:m]
            out[name + "_idx"][k, :o.size] = ik[o]
            out[name + "_score"][k, :o.size] = sk[o]
    return out
