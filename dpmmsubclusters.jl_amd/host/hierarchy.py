"""The agglomerative hierarchy of a model's clusters from their overlap matrix (host/score.py `Predictor.overlap`), in numpy.

O[k][j] = sum_i p_ik p_ij is closed under merging: the model with clusters a and b merged has probabilities p_ia + p_ib, so its overlap
matrix is O with rows and columns a and b added.  The whole hierarchy therefore follows from the K x K matrix (K <= 1024) without
another pass over the data:

  similarity   s(a, b) = O[a][b] / sqrt(O[a][a] O[b][b]), 0 if either diagonal entry is 0 -- the cosine of the two columns of probabilities;
  a step       merges the pair with the largest s, ties to the lexicographically smallest (a, b), a < b; the merged group keeps index a
               (so a group is always represented by its smallest member), row and column b are added into a --
               O[a][a] <- O[a][a] + 2 O[a][b] + O[b][b] -- mass and count likewise, and b leaves the matrix.
"""
import collections

import numpy as np

from .score import Overlap


def _as_overlap(overlap):
    if isinstance(overlap, Overlap) or all(hasattr(overlap, f) for f in ("matrix", "mass", "count", "skipped")):
        O = np.array(overlap.matrix, np.float64)
        mass, count, skipped = np.array(overlap.mass, np.float64), np.array(overlap.count, np.int64), int(overlap.skipped)
    else:
        O = np.array(overlap, np.float64)
        mass, count, skipped = (O.sum(1) if O.ndim == 2 else None), None, 0      # rows of probabilities sum to 1: the row sums are the masses
    if O.ndim != 2 or O.shape[0] != O.shape[1] or O.shape[0] < 1:
        raise ValueError("the overlap matrix must be square, K x K with K >= 1")
    K = O.shape[0]
    if count is None:
        count = np.zeros(K, np.int64)
    if mass.shape != (K,) or count.shape != (K,):
        raise ValueError("mass and count must have one entry per cluster")
    if not np.isfinite(O).all() or (O < 0).any():
        raise ValueError("the overlap matrix must be finite and non-negative")
    return Overlap(O, mass, count, skipped)


def _similarity_row(O, d, a, active):
    """s(a, j) for every j, 0 where a diagonal entry is 0, -inf where j is not active or is a."""
    den = np.sqrt(d[a] * d)
    with np.errstate(all="ignore"):
        s = np.where(den > 0, O[a] / np.where(den > 0, den, 1.0), 0.0)
    s[~active] = -np.inf
    s[a] = -np.inf
    return s


class MergeTree(collections.namedtuple("MergeTree", "merges similarity Z base")):
    """What `merge_tree` returns.

      merges       (K - 1, 2) int64: the 1-based original cluster ids of the two representatives (a < b) of every merge, in order;
      similarity   (K - 1,) float64: the s of every merge;
      Z            (K - 1, 4) float64: the linkage array scipy.cluster.hierarchy.dendrogram reads -- node ids (clusters 0 .. K - 1, the
                   node of merge t is K + t), the distance 1 - s (clipped at 0) and the number of clusters below the node.  The distance
                   need NOT be monotone along the merges: adding two columns of probabilities can bring the sum closer to a third than
                   either was, so a dendrogram may show inversions;
      base         the `Overlap` the tree was built from.
    """
    __slots__ = ()

    @property
    def K(self):
        return self.base.matrix.shape[0]

    def _steps(self, groups, similarity):
        if (groups is None) == (similarity is None):
            raise ValueError("give exactly one of groups= and similarity=")
        K = self.K
        if groups is not None:
            g = int(groups)
            if g != groups or not 1 <= g <= K:
                raise ValueError(f"groups must be an integer in 1..{K}")
            return K - g
        t = float(similarity)
        if t != t:
            raise ValueError("similarity must not be NaN")
        below = np.flatnonzero(self.similarity < t)
        return int(below[0]) if below.size else K - 1

    def cut(self, groups=None, similarity=None):
        """(K,) int64: the 1-based group of every cluster after the first K - groups merges (groups=g), or after the merges in front of
        the first one with s < similarity (similarity=t).  Groups are numbered 1 .. g in the order of their smallest member."""
        steps = self._steps(groups, similarity)
        K = self.K
        rep = np.arange(K)
        for a, b in self.merges[:steps] - 1:
            rep[rep == b] = a
        _, out = np.unique(rep, return_inverse=True)      # representatives are smallest members: their order is the groups' order
        return out.astype(np.int64).reshape(K) + 1

    def overlap(self, groups=None, similarity=None):
        """The coarsened `Overlap`: the merges replayed on matrix, mass and count (one addition per entry and merge), rows and columns in
        the order of `cut`'s group numbers.  It is the overlap matrix of the probabilities summed per group."""
        steps = self._steps(groups, similarity)
        O, mass, count = self.base.matrix.copy(), self.base.mass.copy(), self.base.count.copy()
        keep = np.ones(self.K, bool)
        for a, b in self.merges[:steps] - 1:
            O[a, :] += O[b, :]
            O[:, a] += O[:, b]
            mass[a] += mass[b]
            count[a] += count[b]
            keep[b] = False
        return Overlap(np.ascontiguousarray(O[np.ix_(keep, keep)]), mass[keep], count[keep], self.base.skipped)

    def relabel(self, labels, groups=None, similarity=None):
        """1-based cluster labels (numpy array or torch tensor, any shape) mapped through the cut: the group of every point, an int64
        array / tensor on the input's device."""
        table = self.cut(groups=groups, similarity=similarity)
        if hasattr(labels, "device") and hasattr(labels, "dtype") and not isinstance(labels, np.ndarray):
            import torch
            idx = labels.to(torch.int64)
            if idx.numel() and (int(idx.min()) < 1 or int(idx.max()) > self.K):
                raise ValueError(f"labels must lie in 1..{self.K}")
            return torch.as_tensor(table, device=labels.device)[idx - 1]
        idx = np.asarray(labels)
        if idx.dtype.kind not in "iu":
            raise ValueError("labels must be integers")
        if idx.size and (idx.min() < 1 or idx.max() > self.K):
            raise ValueError(f"labels must lie in 1..{self.K}")
        return table[idx.astype(np.int64) - 1]


def merge_tree(overlap):
    """The `MergeTree` of an `Overlap` (or of a K x K overlap matrix: the masses are then its row sums, the counts 0): K - 1 merges by
    the rule in this module's description.  O(K^3) numpy at worst, K <= 1024."""
    base = _as_overlap(overlap)
    O = base.matrix.copy()
    K = O.shape[0]
    active = np.ones(K, bool)
    d = O.diagonal().copy()
    S = np.full((K, K), -np.inf)                       # s(a, b) in the upper triangle, -inf elsewhere and for clusters that left
    upper = np.triu(np.ones((K, K), bool), 1)
    for a in range(K):
        S[a] = np.where(upper[a], _similarity_row(O, d, a, active), -np.inf)
    merges = np.zeros((K - 1, 2), np.int64)
    sim = np.zeros(K - 1, np.float64)
    Z = np.zeros((K - 1, 4), np.float64)
    node = np.arange(K, dtype=np.int64)                # scipy's node id of the group in slot a
    size = np.ones(K, np.int64)
    for t in range(K - 1):
        a, b = divmod(int(np.argmax(S)), K)            # the first maximum in row-major order: the smallest (a, b)
        s = S[a, b]
        merges[t] = (a + 1, b + 1)
        sim[t] = s
        Z[t] = (min(node[a], node[b]), max(node[a], node[b]), max(0.0, 1.0 - s), size[a] + size[b])
        O[a, :] += O[b, :]
        O[:, a] += O[:, b]
        d[a] = O[a, a]
        active[b] = False
        node[a], size[a] = K + t, size[a] + size[b]
        S[b, :] = -np.inf
        S[:, b] = -np.inf
        row = _similarity_row(O, d, a, active)
        S[a, a + 1:] = row[a + 1:]
        S[:a, a] = row[:a]
    return MergeTree(merges, sim, Z, base)
