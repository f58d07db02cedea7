"""The definitions of include/dpmm_hip_overlap.h in numpy Float64, written from a (K, n) Float32 table.

  lab_i, M_i   as tests/tools/rank_ref.py: Julia's argmax and the maximum with NaN skipped
  a point takes part iff its row holds no NaN and M_i is finite; the others are counted in `skipped` and add nothing
  p_ik         Float32: expf(table[k][i] - M_i) / S_i, S_i the Float32 sum of the numerators in increasing k
  overlap[k][j] = sum_i (double)p_ik (double)p_ij,  mass[k] = sum_i (double)p_ik,  count[k] = #{i takes part, lab_i == k + 1}
Two Float64 summations of n non-negative terms agree within a relative n * 2^-52 (`bound`): the tolerance of every comparison.
(numpy's Float32 exp may differ from the device's expf in the last bit: GPU tests take p from `predict` and use `from_probs`.)"""
import numpy as np

from . import rank_ref


def bound(n):
    return max(int(n), 1) * 2.0 ** -52


def probs(table):
    """((n, K) float32 probabilities with zero rows for the points that take no part, lab (n,), part (n,))."""
    table = np.asarray(table, np.float32)
    K, n = table.shape
    lab, M, part = rank_ref.labels_and_scores(table)
    P = np.zeros((n, K), np.float32)
    if part.any():
        with np.errstate(all="ignore"):
            e = np.exp((table[:, part] - M[part][None, :]).astype(np.float32)).astype(np.float32)      # (K, n_part)
        S = np.zeros(e.shape[1], np.float32)
        for k in range(K):
            S = (S + e[k]).astype(np.float32)
        P[part] = (e / S[None, :]).astype(np.float32).T
    return P, lab, part


def from_probs(P, lab, part=None):
    """dict(overlap, mass, count, skipped) of (n, K) Float32 probabilities and 1-based labels; part: who takes part (default: rows without NaN)."""
    P = np.asarray(P)
    assert P.dtype == np.float32
    n, K = P.shape
    part = ~np.isnan(P).any(1) if part is None else np.asarray(part, bool)
    Q = P[part].astype(np.float64)
    return dict(overlap=Q.T @ Q, mass=Q.sum(0), count=np.bincount(np.asarray(lab)[part] - 1, minlength=K).astype(np.int64)[:K],
                skipped=int(n - part.sum()))


def overlap(table, n_valid=None):
    """The definitions on the first n_valid columns of a (K, n) Float32 table."""
    table = np.asarray(table, np.float32)
    table = table[:, :table.shape[1] if n_valid is None else int(n_valid)]
    P, lab, part = probs(table)
    return from_probs(P, lab, part)


def add(results):
    """The result for the union of disjoint pieces."""
    return dict(overlap=sum(r["overlap"] for r in results), mass=sum(r["mass"] for r in results), count=sum(r["count"] for r in results),
                skipped=sum(r["skipped"] for r in results))


def close(got, want, n):
    """Every entry of got within the relative bound(n) of want (both non-negative)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and bool(np.all(np.abs(got - want) <= bound(n) * np.maximum(got, want)))
