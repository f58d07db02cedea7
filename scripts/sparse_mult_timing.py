"""Lab script: sweep and statistics-pass kernel times of the Multinomial prior on sparse (CSC) points against the dense path.

   python3 scripts/sparse_mult_timing.py c4 [N]                 C4's data (D = 1000, K = 32, 100 trials), dense and sparse, one process
   python3 scripts/sparse_mult_timing.py wide D K [N] [nnz]     wide vocabulary, `nnz` entries per point (default 100), sparse only

One process, fixed labels and parameters (restored in front of every sweep), 3 warm-up + 20 timed launches, HIP events around the
kernels (DPMM_OPT_KERNEL_TIMING through the binding's Worker); prints median, min and max per kernel, the algorithmic HBM bytes of a
sweep (entries + pointers + labels) and its gather volume nnz (K + 2) 4 B.  Run each invocation under its own `timeout`."""
import subprocess
import sys

import numpy as np

sys.path.insert(0, ".")
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
WARM, REPS = 3, 20


def commit():
    try:
        return subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "?"
    except Exception:  # noqa: BLE001
        return "?"


def time_worker(wk, y, sub, K, D, name, nnz_total, n):
    wk.set_labels(y, sub); wk.set_num_clusters(K)
    pk = wk.suffstats_packed()
    l, r = pk[0::2, 1:], pk[1::2, 1:]
    rows = np.stack([l + r, l, r], axis=1).reshape(3 * K, D) + 1.0
    logp = np.log(rows / rows.sum(1, keepdims=True)).astype(np.float32)
    lr = np.full((K, 2), 0.5, np.float32); w = np.full(K, 1.0 / K, np.float32)
    sw, st = [], []
    for it in range(WARM + REPS):
        wk.set_labels(y, sub)
        wk.suffstats_packed()
        st.append(wk.last_kernel_ms()[1])
        wk.set_params_mult(logp, lr, w)
        wk.sweep(it + 1)
        sw.append(wk.last_kernel_ms()[0])
    lab, _ = wk.get_labels()
    sw, st = np.array(sw[WARM:]), np.array(st[WARM:])
    line = (f"{name}: sweep median {np.median(sw):.4f} ms (min {sw.min():.4f}, max {sw.max():.4f}); statistics median {np.median(st):.4f} ms "
            f"(min {st.min():.4f}, max {st.max():.4f}); labels equal to the start {np.mean(lab == y):.4f}")
    if nnz_total:
        alg = nnz_total * 6 + (n + 1) * 8 + n * 4
        gather = nnz_total * (K + 2) * 4
        t = np.median(sw) * 1e-3
        line += (f"\n    algorithmic HBM bytes per sweep {alg / 1e6:.1f} MB ({alg / t / 1e9:.0f} GB/s at the median); gather volume "
                 f"{gather / 1e9:.2f} GB ({gather / t / 1e12:.2f} TB/s)")
    print(line, flush=True)
    return lab


def to_csc(X):
    r, c = np.nonzero(X)
    cp = np.zeros(X.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=X.shape[0]), out=cp[1:])
    return cp, c.astype(np.int64), X[r, c].astype(np.float32)


def c4(N):
    import torch
    import bench
    D, K = 1000, 32
    X, y = bench.gpu_multinomial_mixture(torch, N, D, K, 100, 12345)
    sub = 1 + np.random.default_rng(0).integers(0, 2, N)
    wk = pkg.Worker(pkg.PRIOR_MULT, D, N, device=0, seed=123456789)
    torch.cuda.synchronize()
    wk.upload_points_device(X.data_ptr(), X.stride(0))
    ld = time_worker(wk, y, sub, K, D, "dense (byte path)", 0, N)
    wk.close()
    cp = np.zeros(N + 1, np.int64); rv, nz = [], []
    for a in range(0, N, 100000):                                 # the host copy in blocks: 4 GB dense at N = 1e6
        c, r, v = to_csc(X[a:a + 100000].cpu().numpy())
        cp[a + 1:a + 1 + len(c) - 1] = cp[a] + c[1:]; rv.append(r); nz.append(v)
    rv, nz = np.concatenate(rv), np.concatenate(nz)
    del X
    torch.cuda.empty_cache()
    wk = pkg.Worker(pkg.PRIOR_MULT, D, N, device=0, seed=123456789)
    wk.upload_points_csc(cp, rv, nz)
    ls = time_worker(wk, y, sub, K, D, f"sparse ({len(rv) / N:.1f} entries per point)", len(rv), N)
    wk.close()
    print(f"labels of the last sweep, sparse against dense: {int((ld != ls).sum())} of {N} differ")


def wide(D, K, N, per):
    rng = np.random.default_rng(1)
    y = rng.integers(1, K + 1, N)
    blk = D // K
    words = np.where(rng.random((N, per)) < 0.9, (y - 1)[:, None] * blk + rng.integers(0, min(400, blk), (N, per)), rng.integers(0, D, (N, per)))
    words.sort(axis=1)
    first = np.ones_like(words, bool); first[:, 1:] = words[:, 1:] != words[:, :-1]
    cp = np.zeros(N + 1, np.int64); np.cumsum(first.sum(1), out=cp[1:])
    rv = words[first].astype(np.int64)
    nz = np.diff(np.append(np.flatnonzero(first.ravel()), words.size)).astype(np.float32)
    sub = 1 + rng.integers(0, 2, N)
    wk = pkg.Worker(pkg.PRIOR_MULT, D, N, device=0, seed=123456789)
    wk.upload_points_csc(cp, rv, nz)
    time_worker(wk, y, sub, K, D, f"sparse D={D} K={K} N={N} ({len(rv) / N:.1f} entries per point)", len(rv), N)
    wk.close()


if __name__ == "__main__":
    print(f"build: commit {commit()}", flush=True)
    if sys.argv[1] == "c4":
        c4(int(float(sys.argv[2])) if len(sys.argv) > 2 else 10 ** 6)
    else:
        wide(int(sys.argv[2]), int(sys.argv[3]), int(float(sys.argv[4])) if len(sys.argv) > 4 else 10 ** 6, int(sys.argv[5]) if len(sys.argv) > 5 else 100)
