"""The posterior summary (host/summary.py) restated in plain numpy: every public field of a PosteriorSummary from `sample(j)` alone.
Shared by tests/test_summary_cpu.py and tests/test_gpu_summary.py."""
import numpy as np


def vi_numpy(C):
    """H_a + H_b - 2 I from a table, natural log; written independently of the product's function."""
    p = C / C.sum()
    pa, pb = p.sum(1), p.sum(0)
    h = lambda q: -sum(v * np.log(v) for v in q if v > 0)      # noqa: E731
    mi = sum(p[i, j] * np.log(p[i, j] / (pa[i] * pb[j])) for i in range(p.shape[0]) for j in range(p.shape[1]) if p[i, j] > 0)
    return h(pa) + h(pb) - 2 * mi


def binder_numpy(za, zb):
    """The share of ordered pairs on which two labellings disagree, from cluster sizes (pair counting, in Python integers)."""
    N = len(za)
    sq = lambda v: sum(int(c) ** 2 for c in np.unique(v, return_counts=True)[1])      # noqa: E731
    both = sum(int(c) ** 2 for c in np.unique(np.stack([za, zb]), axis=1, return_counts=True)[1])
    return (sq(za) + sq(zb) - 2 * both) / (N * N)


def check_summary_recomputes(sm, T, N, iters, final_labels):
    """Every public field of a PosteriorSummary from `sm.sample(j)` alone.  Arrays may be tensors: they are brought to numpy first."""
    host_of = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)      # noqa: E731
    z = [host_of(sm.sample(j)) for j in range(T + 1)]
    assert all(v.shape == (N,) and v.dtype == np.int64 and v.min() >= 1 for v in z)
    assert np.array_equal(z[T], host_of(final_labels))
    assert sm.iterations[T] == iters and len(sm.iterations) == T + 1
    assert sm.num_clusters.shape == (T + 1,) and all(z[j].max() <= sm.num_clusters[j] for j in range(T + 1))
    assert sm.pairwise_vi.shape == sm.pairwise_binder.shape == (T + 1, T) and sm.pairwise_vi.dtype == np.float64
    for j in range(T + 1):
        for s in range(T):
            C = np.zeros((z[j].max(), z[s].max()))
            np.add.at(C, (z[j] - 1, z[s] - 1), 1)
            assert abs(sm.pairwise_vi[j, s] - vi_numpy(C)) < 1e-12, (j, s)
            assert abs(sm.pairwise_binder[j, s] - binder_numpy(z[j], z[s])) < 1e-15, (j, s)
    assert np.array_equal(sm.expected_vi, sm.pairwise_vi.mean(1)) and np.array_equal(sm.expected_binder, sm.pairwise_binder.mean(1))
    for loss, exp in (("vi", sm.expected_vi), ("binder", sm.expected_binder)):
        assert sm.choose(loss) is sm and sm.loss == loss
        assert sm.index == int(np.argmin(exp)) and exp[sm.index] == exp.min() and not np.any(exp[:sm.index] == exp.min())
        lab, conf = host_of(sm.labels), host_of(sm.confidence)
        assert np.array_equal(lab, z[sm.index]) and conf.shape == (N,) and conf.dtype == np.float32
        # the mean over the samples of the share of i's cluster-mates in `labels` that sit in i's cluster of the sample, in Float64
        want = np.zeros(N)
        size = np.bincount(lab)[lab]
        for s in range(T):
            both = np.zeros((lab.max() + 1, z[s].max() + 1))
            np.add.at(both, (lab, z[s]), 1)
            want += both[lab, z[s]] / size
        want /= T
        assert np.abs(conf.astype(np.float64) - want).max() <= (T + 2) * 2.0 ** -24
        assert conf.min() > 0 and conf.max() <= 1
        stable = [k for k in np.unique(lab) if all(len(np.unique(z[s][lab == k])) == 1 and np.sum(z[s] == z[s][lab == k][0]) == np.sum(lab == k)
                                                   for s in range(T))]
        for k in stable:                                             # a cluster that is the same set of points in all samples
            assert np.all(conf[lab == k] == 1.0), k
    return z, stable
