"""Float64 reference of the Multinomial sweep tables and a host-side prediction of the route a tile takes through the sweep kernels.

Reference (what tests/test_gpu_mult_variants.py compares the kernels with):
  table[k][i]      = x_i . logp[3k]       + log w[k]          cluster-level values   (debug_loglik / predict)
  sub[2k + s][i]   = x_i . logp[3k+1+s]   + log lr[k][s]      sub-cluster values     (debug_subloglik)
in numpy Float64 from the Float32 inputs.  TABLE_RTOL / TABLE_ATOL are the project's tolerance for this table (header of
tests/test_gpu_mult.py): a Float32 contraction over D terms in another order -- it does not depend on the number of clusters.

Route prediction (`u8_routes`, `u8_instantiation`, `bf16_instantiation`): this RESTATES launcher and kernel arithmetic of
csrc/mult_sweep.hip and proves nothing about it.  Its only purpose is to keep a test case from quietly missing the instantiation or
branch it was written for: the tests assert that the counts they rely on are non-zero and print them.  What is restated:
  u8_blocks                     mult_sweep.hip:658-661   NRBc = ceil(K / 16), NRBs = 3K <= 16 ? 0 : ceil(K / 8)
  launch_mult_sweep_u8          mult_sweep.hip:700-711   B from NRBc + min(NRBs, 1) (running chain) or NRBc + NRBs (table mode)
  launch_u8: ltab_ok            mult_sweep.hip:685-687   4 * 256 * K <= 76 KiB (B <= 4) or 152 KiB
  visiting order                mult_sweep.hip:186, 203  the permutation the statistics pass left (stable sort by 2 (label-1) + (sub-1)), else storage order
  need set, block list          mult_sweep.hip:216-227   bit (zp >> 3) & 31 of word zp >> 8 for every previous label zp of the tile
  passes of the first call      mult_sweep.hip:231-232, 328   cnt = NRBc + |need| blocks, B per pass; the LDS table needs cnt <= B
  miss set, second call         mult_sweep.hip:435-436, 441-450   new labels whose block of eight clusters the first call did not evaluate
  launch_mult_sweep_bf16        mult_sweep.hip:737-743, 487-488   NRB = ceil(3K / 16), B in {2, 4, 6, 8}, passes of B row blocks
"""
import numpy as np

TILE = 256
TABLE_RTOL, TABLE_ATOL = 1e-5, 1e-3


# --------------------------------------------------------------------------- Float64 reference
def table_f64(X, logp, w, lr):
    """((K, n), (2K, n)) Float64: cluster-level and sub-cluster values of every point."""
    X64 = np.asarray(X, np.float64)
    L = np.asarray(logp, np.float32).astype(np.float64)
    K = len(w)
    t = L[0::3] @ X64.T + np.log(np.asarray(w, np.float32).astype(np.float64))[:, None]
    t2 = np.empty((2 * K, X64.shape[0]))
    for s in (0, 1):
        t2[s::2] = L[1 + s::3] @ X64.T + np.log(np.asarray(lr, np.float32).astype(np.float64)[:, s])[:, None]
    return t, t2


def assert_table(got, want, what=""):
    err = np.abs(np.asarray(got, np.float64) - want)
    print(f"{what}: max |table - f64| = {err.max():.3e} (max |value| {np.abs(want).max():.1f})")
    np.testing.assert_allclose(got, want, rtol=TABLE_RTOL, atol=TABLE_ATOL, err_msg=what)


def sub_pair(tab2, lab):
    """(2, n): the left / right values of the cluster every point was given (1-based labels)."""
    i = np.arange(tab2.shape[1])
    return np.stack([tab2[2 * (lab - 1), i], tab2[2 * (lab - 1) + 1, i]])


def cdf_edge(t64, u):
    """(dist, bound), each (n,).  The Float32 inverse-CDF draw gives the first k with cw_k >= u s (cw the running sum of exp(t_k - max),
    s the total).  dist: distance from u s to the nearest cumulative sum of the Float64 table (the last one, = s, is no edge: u < 1).
    bound: how far a table within the tolerance delta_k = ATOL + RTOL |t_k| can move that comparison: every exp(t_k - max) by the factor
    exp(+-delta_k), so a cumulative sum by at most sum_k p_k (exp(delta_k) - 1) and u s by at most the same; plus the Float32 rounding
    of the draw itself (K additions, the exponentials, the product u s: (K + 8) 2^-23 s).  Two tables inside the tolerance can give a
    point different labels only where dist <= bound."""
    t64 = np.asarray(t64, np.float64)
    K = t64.shape[0]
    p = np.exp(t64 - t64.max(0))
    c = np.cumsum(p, 0)
    s = c[-1]
    us = np.asarray(u, np.float32).astype(np.float64) * s
    edges = c[:-1] if K > 1 else c
    dist = np.abs(edges - us).min(0)
    delta = TABLE_ATOL + TABLE_RTOL * np.abs(t64)
    bound = 2.0 * (p * np.expm1(delta)).sum(0) + (K + 8) * 2.0 ** -23 * s
    return dist, bound


# --------------------------------------------------------------------------- which code a case reaches
def u8_blocks(K):
    return (K + 15) // 16, (0 if 3 * K <= 16 else (K + 7) // 8)


def u8_instantiation(K, table_mode=False):
    """B of mult_sweep_u8_kernel<B> for K clusters."""
    nrbc, nrbs = u8_blocks(K)
    typical = nrbc + nrbs if table_mode else nrbc + min(nrbs, 1)
    return 2 if typical <= 2 else 4 if typical <= 4 else 6 if typical <= 6 else 8


def u8_lds_table(K, table_mode=False):
    """launch_u8's ltab_ok: the K x 256 cluster-level values of a tile fit the instantiation's LDS."""
    cap = (76 if u8_instantiation(K, table_mode) <= 4 else 152) * 1024
    return 4 * 256 * K <= cap


def bf16_instantiation(K):
    """(B, NRB, row blocks of every pass) of mult_sweep_bf16_kernel<B>."""
    nrb = (3 * K + 15) // 16
    B = 2 if nrb <= 2 else 4 if nrb <= 4 else 6 if nrb <= 6 else 8
    return B, nrb, [min(B, nrb - r) for r in range(0, nrb, B)]


def visiting_order(prev_lab, prev_sub, ordered):
    n = len(prev_lab)
    if not ordered:
        return np.arange(n)
    return np.argsort(2 * (np.asarray(prev_lab) - 1) + (np.asarray(prev_sub) - 1), kind="stable")


def u8_routes(K, prev_lab, prev_sub, new_lab, ordered):
    """Per tile of 256 visited points of one running-chain sweep of the byte kernel (1-based labels before / after the sweep):
    single / multi: tiles whose first call has cnt <= B / cnt > B row blocks; miss: tiles with a second call; need_words / miss_words:
    which 32-bit words of the two block sets got a bit; lds: tiles whose label draw read the LDS table (single and ltab_ok)."""
    nrbc, nrbs = u8_blocks(K)
    B = u8_instantiation(K)
    ltab = u8_lds_table(K)
    order = visiting_order(prev_lab, prev_sub, ordered)
    zp = (np.asarray(prev_lab) - 1)[order]
    zn = (np.asarray(new_lab) - 1)[order]
    out = dict(B=B, tiles=0, single=0, multi=0, miss=0, lds=0, need_words=set(), miss_words=set(), max_cnt=0, max_miss=0)
    for t0 in range(0, len(order), TILE):
        need = set((zp[t0:t0 + TILE] >> 3).tolist()) if nrbs else set()
        miss = set((zn[t0:t0 + TILE] >> 3).tolist()) - need if nrbs else set()
        cnt = nrbc + len(need)
        out["tiles"] += 1
        out["single" if cnt <= B else "multi"] += 1
        out["lds"] += int(cnt <= B and ltab)
        out["miss"] += int(bool(miss))
        out["need_words"] |= {j >> 5 for j in need}
        out["miss_words"] |= {j >> 5 for j in miss}
        out["max_cnt"] = max(out["max_cnt"], cnt)
        out["max_miss"] = max(out["max_miss"], len(miss))
    return out


def describe(r):
    return (f"<{r['B']}> tiles {r['tiles']}: first call single-pass {r['single']} (LDS table {r['lds']}), multi-pass {r['multi']} (most blocks {r['max_cnt']}); "
            f"second call {r['miss']} (most blocks {r['max_miss']}); need words {sorted(r['need_words'])}, miss words {sorted(r['miss_words'])}")
