"""Posterior summary of a chain: a consensus clustering and a per-point confidence from label samples kept on the GPU
(include/dpmm_hip_trace.h, csrc/trace.hip).  No reference counterpart: the reference hands back the labels after its last sweep.

`fit(..., keep_samples=T, thin=t, loss="vi")` records the labels of T sweeps -- `i_end - (T-1-j) * t` for j = 0..T-1, `i_end = iters -
argmax_sample_stop - 1` the last sweep that still SAMPLES its labels -- into slots 0..T-1 of the worker's trace, and the final labels
(`dp_model.labels`) into slot T.  Every slot is a CANDIDATE for the point estimate; its expected loss is the mean of its loss against the
T samples:
    vi      Variation of Information, H_a + H_b - 2 I, natural log (Wade & Ghahramani 2018) -- `nmi_vi_from_contingency(C)[1]`
    binder  Binder's loss (Dahl 2006, least-squares clustering): the share of ordered point pairs on which two labellings disagree,
            (sum_a n_a^2 + sum_b n_b^2 - 2 sum_ab n_ab^2) / N^2, from exact integer sums
and the estimate is the candidate with the smallest expected loss, the lower slot on a tie (a sample beats the final labelling).  Both
losses are functions of the contingency table of two labellings and of nothing else, so cluster numbers that change under split, merge
and remove_empty need no alignment.  The tables are Int64 and go through `comm.reduce_counts`: shards add up exactly.

A worker without `trace_*` methods (test stand-ins, third-party factories) is served by numpy: `get_labels()` per recorded sweep and
`np.bincount(a * K_t + b)` per table."""
import numpy as np

from .sampler import nmi_vi_from_contingency

LOSSES = ("vi", "binder")
MAX_SAMPLES = 4095            # DPMM_TRACE_MAX_SLOTS - 1: the final labels take a slot too


def schedule(iters, first_iter, argmax_sample_stop, keep_samples, thin):
    """The sweeps recorded into slots 0..T-1.  ValueError when the first of them would lie before `first_iter`."""
    T, thin = int(keep_samples), int(thin)
    i_end = int(iters) - int(argmax_sample_stop) - 1
    its = [i_end - (T - 1 - j) * thin for j in range(T)]
    if its[0] < first_iter:
        need = int(first_iter) + int(argmax_sample_stop) + 1 + (T - 1) * thin
        raise ValueError(f"keep_samples={T}, thin={thin} would record sweep {its[0]}, before the first sweep {first_iter} of this run: "
                         f"iters must be at least {need}")
    return its


def check_arguments(keep_samples, thin, loss):
    if int(keep_samples) != keep_samples or not 0 <= keep_samples <= MAX_SAMPLES:
        raise ValueError(f"keep_samples must be an integer in 0..{MAX_SAMPLES}")
    if int(thin) != thin or thin < 1:
        raise ValueError("thin must be an integer >= 1")
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {LOSSES}, not {loss!r}")


def pair_list(T):
    """The tables a summary of T samples needs: (j, s) for every candidate j in 0..T against every sample s < j, then the diagonals
    (cluster sizes).  A candidate's table against a LATER sample is the transpose of that sample's against it."""
    return [(j, s) for j in range(T + 1) for s in range(min(j, T))] + [(j, j) for j in range(T + 1)]


def contingency(za, zb, Ka, Kb):
    """C[a][b] = #{i : za_i = a, zb_i = b} for 0-based ids; an id >= K of its side is counted nowhere (as the kernels ignore it)."""
    za, zb = np.asarray(za, np.int64), np.asarray(zb, np.int64)
    ok = (za >= 0) & (za < Ka) & (zb >= 0) & (zb < Kb)
    return np.bincount(za[ok] * Kb + zb[ok], minlength=Ka * Kb).reshape(Ka, Kb).astype(np.int64)


def _sum_of_squares(a):
    a = np.asarray(a, np.int64).ravel()
    if a.size == 0:
        return 0
    if int(a.max()) < 2 ** 31 and int(a.sum()) < 2 ** 31:
        return int((a * a).sum())                                   # below 2^62: exact in Int64
    return sum(int(v) * int(v) for v in a[a != 0])                  # Python integers


def binder_from_contingency(C):
    """Binder's loss of the two labellings behind an Int64 contingency table: the share of ordered pairs (i, i') co-clustered in exactly
    one of them.  Integer sums, one division."""
    C = np.asarray(C, np.int64)
    N = int(C.sum())
    if N == 0:
        return 0.0
    return (_sum_of_squares(C.sum(1)) + _sum_of_squares(C.sum(0)) - 2 * _sum_of_squares(C)) / (N * N)


def loss_matrices(tables, T):
    """tables: {(j, s): Int64 table} over `pair_list(T)`, summed over the shards.  -> (vi, binder), both (T + 1, T) Float64: row j the
    candidate, column s the sample."""
    vi, binder = np.zeros((T + 1, T)), np.zeros((T + 1, T))
    for j in range(T + 1):
        for s in range(T):
            if j == s:
                continue                                            # a labelling against itself: both losses are 0
            C = tables[(j, s)] if j > s else tables[(s, j)].T
            vi[j, s] = max(0.0, nmi_vi_from_contingency(C)[1])      # (H_a + H_b - 2 I of equal partitions may round below 0)
            binder[j, s] = binder_from_contingency(C)
    return vi, binder


def select(expected):
    """The candidate with the smallest expected loss; the lower slot on a tie."""
    return int(np.argmin(np.asarray(expected, np.float64)))


def ratio_tables(tables, anchor, T):
    """For every sample s the Float32 table C[a][b] / n_a of the anchor's clusters a against the sample's b: the share of cluster a that
    sits in b.  Float64 division, rounded once; an empty cluster's row is 0."""
    n_a = np.diag(tables[(anchor, anchor)]).astype(np.float64)
    out = []
    for s in range(T):
        C = tables[(anchor, s)] if anchor >= s else tables[(s, anchor)].T
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(n_a[:, None] > 0, np.asarray(C, np.float64) / n_a[:, None], 0.0)
        out.append(np.ascontiguousarray(r, np.float32))
    return out


def confidence_numpy(z_anchor, z_samples, ratio):
    """What dpmm_trace_confidence computes, operation for operation: Float32 sum in the order listed, one Float32 division."""
    za = np.asarray(z_anchor, np.int64)
    acc = np.zeros(za.shape, np.float32)
    for zs, r in zip(z_samples, ratio):
        zs = np.asarray(zs, np.int64)
        ok = (za < r.shape[0]) & (zs < r.shape[1])
        acc = acc + np.where(ok, r[np.where(ok, za, 0), np.where(ok, zs, 0)], np.float32(0)).astype(np.float32)
    return (acc / np.float32(len(ratio))).astype(np.float32)


class _Local:
    """What `comm.gather_labels` reads of a worker, around one local vector."""
    def __init__(self, a):
        self.a = a

    def get_labels(self):
        return self.a, self.a


class TraceRecorder:
    """The `on_iteration` hook that fills the trace, and afterwards its reader.  `inner`: another hook to call first (checkpoints)."""

    def __init__(self, sampler, iterations, inner=None):
        self.sampler, self.wk, self.comm, self.inner = sampler, sampler.wk, sampler.comm, inner
        self.T = len(iterations)
        self.iterations = list(iterations)
        self.slot_of = {it: j for j, it in enumerate(self.iterations)}
        self.K = [0] * (self.T + 1)
        self.native = all(hasattr(self.wk, m) for m in ("trace_open", "trace_record", "trace_tables", "trace_confidence", "trace_read"))
        if self.native:
            self.wk.trace_open(self.T + 1)
        else:
            self.ids = [None] * (self.T + 1)                      # 0-based ids of the shard per slot

    def __call__(self, i, sampler):
        if self.inner is not None:
            self.inner(i, sampler)
        j = self.slot_of.get(i)
        if j is not None:
            self.record(j, sampler.K)

    def record(self, slot, K):
        if self.native:
            self.wk.trace_record(slot, K)
        else:
            self.ids[slot] = np.asarray(self.wk.get_labels()[0], np.int64) - 1
        self.K[slot] = int(K)

    def finish(self, iters):
        """After the loop: the final labels into slot T."""
        self.record(self.T, self.sampler.K)
        self.iterations.append(int(iters))

    # ---- reading
    def tables(self, pairs):
        """{pair: table} summed over the ranks: one `reduce_counts` of all tables, packed."""
        if self.native:
            local = self.wk.trace_tables(pairs)
        else:
            local = [contingency(self.ids[s], self.ids[t], self.K[s], self.K[t]) for s, t in pairs]
        flat = np.concatenate([t.ravel() for t in local]) if local else np.zeros(0, np.int64)
        flat = np.asarray(self.comm.reduce_counts(flat), np.int64)
        out, off = {}, 0
        for (s, t), loc in zip(pairs, local):
            out[(s, t)] = flat[off:off + loc.size].reshape(loc.shape)
            off += loc.size
        return out

    def _result(self, device_call, host_call):
        """A vector over the whole data set, in the type `_final_labels` gives the labels."""
        dev = getattr(self.sampler, "data_device", None)
        if dev is not None and self.native and getattr(self.comm, "world", 1) == 1:
            return device_call(dev)
        whole = self.comm.gather_labels(_Local(host_call()))[0]
        if dev is None:
            return whole
        import torch
        return torch.from_numpy(np.ascontiguousarray(whole)).to(dev)

    def read(self, slot):
        if self.K[slot] == 0:
            raise IndexError(f"slot {slot} was not recorded")
        if self.native:
            return self._result(lambda dev: self.wk.trace_read(slot, device=dev), lambda: self.wk.trace_read(slot))
        return self._result(None, lambda: self.ids[slot] + 1)

    def confidence(self, anchor, ratio):
        slots = list(range(self.T))
        if self.native:
            return self._result(lambda dev: self.wk.trace_confidence(anchor, slots, ratio, device=dev),
                                lambda: self.wk.trace_confidence(anchor, slots, ratio))
        return self._result(None, lambda: confidence_numpy(self.ids[anchor], [self.ids[s] for s in slots], ratio))


class PosteriorSummary:
    """Point estimate and uncertainty from the T kept label samples of a chain (`dp_model.summary`).

    index              the chosen slot: 0..T-1 a sample, T the final labelling (`dp_model.labels`)
    iterations         the sweep recorded in each slot; `iters` for slot T
    num_clusters       (T + 1,) clusters of each slot
    pairwise_vi, pairwise_binder     (T + 1, T) Float64: loss of candidate j against sample s
    expected_vi, expected_binder     (T + 1,) their row means, the posterior expected loss of each candidate
    loss               "vi" or "binder": which of the two chose `index`
    labels             Int64, 1-based, the labelling of slot `index` IN THE NUMBERING OF THAT SWEEP.  Unless `index == T` this is not
                       the numbering of `dp_model.sampler`'s clusters (split, merge and remove_empty renumber between sweeps): use
                       it as a partition, not as an index into the fitted clusters.
    confidence         Float32 (N,), in (0, 1]: the mean over the T samples of the share of point i's cluster-mates in `labels`
                       (itself included) that share i's cluster in that sample -- the posterior co-clustering probability of i,
                       averaged over its cluster.  1 for a cluster that is identical in all samples.
    `labels`, `confidence` and `sample(j)` are tensors on the data's device when the data was a device tensor, numpy arrays otherwise,
    as `dp_model.labels` is.  The trace they are read from lives as long as the model's worker."""

    def __init__(self, trace, loss="vi"):
        self._trace = trace
        T = self.T = trace.T
        self.iterations = list(trace.iterations)
        self.num_clusters = np.asarray(trace.K, np.int64)
        self._tables = trace.tables(pair_list(T))
        self.pairwise_vi, self.pairwise_binder = loss_matrices(self._tables, T)
        self.expected_vi, self.expected_binder = self.pairwise_vi.mean(1), self.pairwise_binder.mean(1)
        self.choose(loss)

    def choose(self, loss):
        """Selects again under `loss` from the kept matrices; recomputes `labels` and `confidence`."""
        if loss not in LOSSES:
            raise ValueError(f"loss must be one of {LOSSES}, not {loss!r}")
        self.loss = loss
        self.index = select(self.expected_vi if loss == "vi" else self.expected_binder)
        self.labels = self._trace.read(self.index)
        self.confidence = self._trace.confidence(self.index, ratio_tables(self._tables, self.index, self.T))
        return self

    def sample(self, j):
        """The labels of slot j (0..T-1 the samples, T the final labelling), 1-based, in that sweep's numbering."""
        j = int(j)
        if not 0 <= j <= self.T:
            raise IndexError(f"slot {j} is outside 0..{self.T}")
        return self._trace.read(j)
