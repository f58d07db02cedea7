// Stand-alone check of csrc/stats_ranges.h (built and run by tests/test_stats_ranges_cpu.py, under ASan + UBSan where the compiler has
// them; links nothing of ROCm).  The header's four functions are evaluated by two kernels that never talk to each other: niw_stats_kernel
// WRITES one slab per segment of a workgroup's item range, niw_reduce_kernel READS, per bin, the slabs it believes the bin has.  This
// program walks a layout of items both ways and compares: a slot written and not read is a segment of points lost, a slot read and not
// written is stale memory added to a row, and neither shows in a sum unless a test's shapes happen to cross the boundary.
#include "../../dpmmsubclusters.jl_amd/csrc/stats_ranges.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

using namespace dpmm;

static long g_bad = 0, g_layouts = 0;
static const char *g_what = "";
static int g_T = 0, g_groups = 0, g_nbins = 0;
#define CHECK(x) do { if (!(x)) { if (g_bad < 20) std::fprintf(stderr, "stats_ranges_check: line %d: %s  [%s: T=%d groups=%d nbins=%d]\n", \
                                                                __LINE__, #x, g_what, g_T, g_groups, g_nbins); ++g_bad; } } while (0)

// items[b] = work items of bin b (0: an empty bin).  One layout, one `groups` (the grid of the statistics kernel).
static void check_layout(const std::vector<int> &items, int groups) {
    const int nbins = (int)items.size();
    std::vector<int> item_start(nbins + 1, 0);
    for (int b = 0; b < nbins; ++b) item_start[b + 1] = item_start[b] + items[b];
    const int T = item_start[nbins];
    g_T = T; g_groups = groups; g_nbins = nbins; ++g_layouts;
    if (groups > NIW_STATS_MAX_GROUPS) groups = NIW_STATS_MAX_GROUPS;      // launch_niw_stats
    const int G = std::min(groups, T);                                      // both kernels
    const size_t nslots = (size_t)NIW_STATS_MAX_GROUPS + (size_t)nbins;     // the slabs the context holds
    // (kept between layouts and cleared by the list of slots touched: most layouts use a handful of the 4096 + nbins slots)
    static std::vector<int> w_bin, w_items, reads;
    static std::vector<size_t> touched;
    if (w_bin.size() < nslots) { w_bin.resize(nslots, -1); w_items.resize(nslots, 0); reads.resize(nslots, 0); }
    // ---- the writer: niw_stats_kernel, workgroup w of G
    long long covered = 0;
    for (int w = 0; w < G; ++w) {
        const int it0 = range_bound(w, T, G), it1 = range_bound(w + 1, T, G);
        CHECK(it1 > it0);                                                   // every workgroup range is non-empty
        CHECK(it0 >= 0 && it1 <= T);
        if (w == 0) CHECK(it0 == 0);
        if (w == G - 1) CHECK(it1 == T);
        for (int item = it0; item < it1;) {
            // largest b < nbins with item_start[b] <= item (empty bins share a start with their successor: the last one holds the item)
            const int b = (int)(std::upper_bound(item_start.begin(), item_start.begin() + nbins, item) - item_start.begin()) - 1;
            CHECK(b >= 0 && items[b] > 0 && item_start[b] <= item && item < item_start[b + 1]);
            const int e = std::min(it1, item_start[b + 1]);
            const size_t slot = item == it0 ? (size_t)w : (size_t)NIW_STATS_MAX_GROUPS + (size_t)b;
            CHECK(slot < nslots);
            if (slot < nslots) {
                CHECK(w_bin[slot] == -1);                                   // no slot is written twice
                if (w_bin[slot] == -1) touched.push_back(slot);
                w_bin[slot] = b;
                w_items[slot] = e - item;
            }
            covered += e - item;
            item = e;
        }
    }
    CHECK(covered == T);
    // ---- the reader: niw_reduce_kernel, bin b
    for (int b = 0; b < nbins; ++b) {
        const int i0 = item_start[b], i1 = item_start[b + 1];
        if (i1 <= i0) continue;
        int wa = 1, wb = 0;
        range_heads(i0, i1, T, G, wa, wb);
        const int nheads = 1 + std::max(0, wb - wa + 1);
        long long got = 0;
        for (int h = 0; h < nheads; ++h) {
            const long long slot = h == 0 ? head_slot(i0, b, T, G) : wa + h - 1;
            CHECK(slot >= 0 && (size_t)slot < nslots);
            if (slot < 0 || (size_t)slot >= nslots) continue;
            if (h > 0) {                                                    // a boundary strictly inside the bin
                CHECK(slot < G);
                const int B = range_bound((int)slot, T, G);
                CHECK(i0 < B && B < i1);
            }
            CHECK(w_bin[slot] == b);                                        // every slot read was written, for that bin
            CHECK(reads[slot] == 0);                                        // no slot is read twice
            if (w_bin[slot] >= 0) ++reads[slot];                            // (only written slots are cleared after the layout)
            if (w_bin[slot] == b) got += w_items[slot];
        }
        CHECK(got == i1 - i0);                                              // the heads of a bin cover the bin's items
    }
    // ---- the set read equals the set written (a slot read and never written failed above)
    for (size_t s : touched) {
        CHECK(reads[s] == 1);
        w_bin[s] = -1; w_items[s] = 0; reads[s] = 0;
    }
    touched.clear();
}

// range_owner on its own: the w with B(w) <= item < B(w + 1)
static void check_owner(int T, int G, int item) {
    g_T = T; g_groups = G;
    const int w = range_owner(item, T, G);
    CHECK(w >= 0 && w < G);
    CHECK(range_bound(w, T, G) <= item && item < range_bound(w + 1, T, G));
}

static void compositions(int T, int nbins, std::vector<int> &cur, int groups_max) {
    if ((int)cur.size() == nbins - 1) {
        int used = 0;
        for (int v : cur) used += v;
        cur.push_back(T - used);
        for (int groups = 1; groups <= groups_max; ++groups) check_layout(cur, groups);
        cur.pop_back();
        return;
    }
    int used = 0;
    for (int v : cur) used += v;
    for (int v = 0; v <= T - used; ++v) { cur.push_back(v); compositions(T, nbins, cur, groups_max); cur.pop_back(); }
}

int main() {
    std::mt19937_64 rng(20240607);
    auto below = [&](uint64_t m) { return (int64_t)(rng() % m); };
    // T items cut into nbins bins at sorted random points (empty bins where two cuts coincide)
    auto random_cut = [&](int T, int nbins) {
        std::vector<int64_t> cuts(nbins - 1);
        for (auto &c : cuts) c = below((uint64_t)T + 1);
        std::sort(cuts.begin(), cuts.end());
        std::vector<int> items(nbins);
        int64_t prev = 0;
        for (int b = 0; b < nbins; ++b) { const int64_t c = b + 1 < nbins ? cuts[b] : T; items[b] = (int)(c - prev); prev = c; }
        return items;
    };

    // (1) every (T, groups) with T <= 48 and groups <= T + 2: all compositions of T into up to 6 bins while they are few (T <= 9:
    //     2002 of 6 bins at most), a fixed-seed sample of 160 per pair beyond that
    g_what = "small";
    for (int T = 0; T <= 48; ++T) {
        for (int G = 1; G <= T; ++G) for (int item = 0; item < T; ++item) check_owner(T, G, item);
        if (T <= 9) {
            for (int nbins = 1; nbins <= 6; ++nbins) { std::vector<int> cur; compositions(T, nbins, cur, T + 2); }
        } else {
            for (int groups = 1; groups <= T + 2; ++groups)
                for (int rep = 0; rep < 160; ++rep) check_layout(random_cut(T, 1 + (int)below(6)), groups);
        }
    }
    // (2) many bins, most of them small or empty: up to 2048 bins, items per bin from {0, 0, 1, 1, 2, 5, 40}
    g_what = "many bins";
    {
        const int pool[7] = {0, 0, 1, 1, 2, 5, 40};
        const int groups_of[7] = {1, 2, 3, 7, 64, 1024, 4096};
        for (int rep = 0; rep < 400; ++rep) {
            const int nbins = rep < 8 ? 2048 : 1 + (int)below(2048);
            std::vector<int> items(nbins);
            for (auto &v : items) v = pool[below(7)];
            if (rep % 5 == 0) for (int b = 0; b < nbins / 2; ++b) items[(size_t)below(nbins)] = 0;      // long runs of empty bins
            for (int groups : groups_of) check_layout(items, groups);
        }
    }
    // (3) large item counts: T around 2^31 / 64, where w T and (item + 1) G leave 32 bits
    g_what = "large";
    {
        const int T0 = (int)((1ll << 31) / 64);
        const int Ts[] = {T0 - 4097, T0 - 1, T0, T0 + 1, T0 + 4095, 2 * T0 - 1, 2 * T0 + 12345};
        const int groups_of[] = {4096, 5000, 4095, 1, 7};
        for (int T : Ts) {
            for (int groups : groups_of) {
                const int Ge = std::min(std::min(groups, NIW_STATS_MAX_GROUPS), T);
                for (int rep = 0; rep < 64; ++rep) check_owner(T, Ge, rep < 2 ? (rep ? T - 1 : 0) : (int)below((uint64_t)T));
                check_layout(std::vector<int>{T}, groups);
                check_layout(std::vector<int>{0, T - 1, 0, 1, 0}, groups);
                for (int rep = 0; rep < 6; ++rep) check_layout(random_cut(T, 2 + (int)below(63)), groups);
                // bins that start exactly on, one before and one after a workgroup boundary
                std::vector<int> edge;
                int at = 0;
                for (int w : {1, 2, 1000, 2048, 4094, 4095}) {
                    if (w >= Ge) continue;
                    for (int d = -1; d <= 1; ++d) { const int s = range_bound(w, T, Ge) + d; if (s > at) { edge.push_back(s - at); at = s; } }
                }
                edge.push_back(T - at);
                check_layout(edge, groups);
            }
        }
    }
    if (g_bad) { std::fprintf(stderr, "stats_ranges_check: %ld failed checks over %ld layouts\n", g_bad, g_layouts); return 1; }
    std::printf("stats_ranges_check ok: %ld layouts\n", g_layouts);
    return 0;
}
