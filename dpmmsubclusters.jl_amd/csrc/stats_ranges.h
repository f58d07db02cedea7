// stats_ranges.h -- the range partition of the NIW statistics pass (suffstats.hip): which workgroup of niw_stats_kernel accumulates which
// items, which slab slot a segment's sum is written to, and -- evaluated independently by niw_reduce_kernel -- which slots hold the
// segments of a bin.  Plain integer C++ with no device call, so that a host program can walk both sides and compare them
// (tests/tools/stats_ranges_check.cpp).
#pragma once

#if defined(__HIPCC__)
#define STATS_RANGES_HD __device__ __forceinline__
#else
#define STATS_RANGES_HD inline
#endif

namespace dpmm {

constexpr int NIW_STATS_MAX_GROUPS = 4096;   // workgroups of the NIW statistics kernel at most; slab slots = this + 2 K (head_slot)

// Workgroup w owns the contiguous item range [B(w), B(w+1)), B(w) = floor(w T / G) -- T items over G = min(groups, T) workgroups, so
// that two ranges differ by at most ONE item.  (Round 3 cut ranges of q = ceil(T / groups) items: with the derived statistics a pass
// at the 8-GPU shard size has T = 2 200 items for 1 024 groups, q = 3, and 733 workgroups did all the work on a third of the chip
// while the rest had none: 0.124 ms where T / groups of the N = 1e7 pass predicts 0.05.)  Consecutive items of one bin are contiguous
// in perm, so the range splits into one segment per bin it touches; each segment is accumulated in registers and written as ONE
// slab, stored at the slot of its first item (its "head").  Heads of bin b are item_start[b] and every B(w) strictly inside the
// bin -- the reduce kernel walks exactly those (range_bound / range_heads below: both kernels use the same two functions).
STATS_RANGES_HD int range_bound(int w, int T, int G) { return (int)(((long long)w * T) / G); }
// boundaries B(w) with i0 < B(w) < i1: w in [wa, wb] (empty when wb < wa).  B(w) > i0 <=> w T >= (i0 + 1) G;  B(w) < i1 <=> w T < i1 G.
STATS_RANGES_HD void range_heads(int i0, int i1, int T, int G, int &wa, int &wb) {
    wa = (int)((((long long)i0 + 1) * G + T - 1) / T);
    wb = (int)(((long long)i1 * G + T - 1) / T) - 1;
}
// Slab SLOTS (the items used to name them: one 21 KB slab per item id, i.e. n / chunk of them allocated -- which tied the granularity of
// the balance to the memory the context holds): the head at a workgroup boundary B(w) lives in slot w, a head at the start of a bin that
// falls INSIDE a workgroup's range in slot NIW_STATS_MAX_GROUPS + bin.  NIW_STATS_MAX_GROUPS + 2 K slots whatever the item size.
STATS_RANGES_HD int range_owner(int item, int T, int G) { return (int)((((long long)item + 1) * G + T - 1) / T) - 1; }   // w with B(w) <= item < B(w+1)
STATS_RANGES_HD int head_slot(int item, int bin, int T, int G) {
    const int w = range_owner(item, T, G);
    return range_bound(w, T, G) == item ? w : NIW_STATS_MAX_GROUPS + bin;
}

}  // namespace dpmm
