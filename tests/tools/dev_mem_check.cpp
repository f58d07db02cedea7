// Stand-alone check of csrc/dev_mem.h (built and run by tests/test_dev_mem_cpu.py under ASan + UBSan; links no ROCm library).
// The five runtime calls the header makes are counting stand-ins on malloc / free; g_fail_at makes the n-th allocation from now fail.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <set>

static std::set<void *> g_live;
static long g_allocs = 0, g_frees = 0, g_fail_at = 0, g_cleared = 0;
static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "dev_mem_check: line %d: %s\n", __LINE__, #x); ++g_bad; } } while (0)

static hipError_t fake_alloc(void **p, size_t n) {
    if (g_fail_at > 0 && --g_fail_at == 0) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(n ? n : 1);
    g_live.insert(*p);
    ++g_allocs;
    return hipSuccess;
}
static hipError_t fake_free(void *p) {
    if (!p) return hipSuccess;
    CHECK(g_live.erase(p) == 1);      // freed twice, or never allocated
    std::free(p);
    ++g_frees;
    return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void **p, size_t n) { return fake_alloc(p, n); }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { return fake_alloc(p, n); }
hipError_t hipFree(void *p) { return fake_free(p); }
hipError_t hipHostFree(void *p) { return fake_free(p); }
hipError_t hipGetLastError(void) { ++g_cleared; return hipSuccess; }
}

#include "../../dpmmsubclusters.jl_amd/csrc/dev_mem.h"
using namespace dpmm;

template <class Buf> static void owner_checks() {
    {   // alloc over a live block frees the old one exactly once
        Buf b;
        CHECK(b.get() == nullptr && b.bytes == 0);
        CHECK(b.alloc(100) == hipSuccess && b.get() != nullptr && b.bytes == 100 && g_live.size() == 1);
        const long f0 = g_frees;
        void *old = b.get();
        CHECK(b.alloc(200) == hipSuccess && b.bytes == 200);
        CHECK(g_frees == f0 + 1 && g_live.size() == 1 && g_live.count(old) == 0);
        static_cast<char *>(static_cast<void *>(b.get()))[199] = 1;      // the whole block is there (ASan)
        // a failed alloc leaves the owner empty, the error cleared, and nothing of it live
        const long c0 = g_cleared;
        g_fail_at = 1;
        CHECK(b.alloc(300) == hipErrorOutOfMemory && b.get() == nullptr && b.bytes == 0 && g_live.empty() && g_cleared == c0 + 1);
        b.reset();      // an empty owner resets to nothing
        CHECK(g_live.empty());
    }
    {   // a failed alloc of an empty owner: the live count is unchanged
        Buf keep, b;
        CHECK(keep.alloc(8) == hipSuccess);
        g_fail_at = 1;
        CHECK(b.alloc(8) != hipSuccess && b.get() == nullptr && g_live.size() == 1);
    }
    CHECK(g_live.empty());
    {   // move assignment and swap neither leak nor free twice
        Buf a, b;
        CHECK(a.alloc(16) == hipSuccess && b.alloc(32) == hipSuccess);
        void *pa = a.get(), *pb = b.get();
        a.swap(b);
        CHECK(a.get() == pb && a.bytes == 32 && b.get() == pa && b.bytes == 16 && g_live.size() == 2);
        swap(a, b);
        CHECK(a.get() == pa && b.get() == pb);
        a = std::move(b);      // a's block goes, b is empty
        CHECK(a.get() == pb && a.bytes == 32 && b.get() == nullptr && b.bytes == 0 && g_live.size() == 1);
        Buf &self = a;
        a = std::move(self);
        CHECK(a.get() == pb && g_live.size() == 1);
        Buf c(std::move(a));
        CHECK(c.get() == pb && a.get() == nullptr && g_live.size() == 1);
        Buf empty;
        c = std::move(empty);
        CHECK(c.get() == nullptr && g_live.empty());
    }
    CHECK(g_live.empty());
}

// the shape of master_capacity: five owners built beside the old ones; the third allocation fails and the function returns early
static int five_owners(long fail_at) {
    DevBuf<double> fac, mean, kap, nu, rows;
    g_fail_at = fail_at;
    if (fac.alloc(64) != hipSuccess) return 1;
    if (mean.alloc(64) != hipSuccess) return 1;
    if (kap.alloc(64) != hipSuccess) return 1;
    if (nu.alloc(64) != hipSuccess) return 1;
    if (rows.alloc(64) != hipSuccess) return 1;
    return 0;
}

// today's routines, written out: the capacity the loops of the glue gave before there was one routine
static size_t old_capacity(size_t need, size_t floor) { size_t cap = floor; while (cap < need) cap *= 2; return cap; }

int main() {
    owner_checks<DevBuf<float>>();
    owner_checks<PinBuf<char>>();
    owner_checks<DevBuf<void>>();

    CHECK(five_owners(3) == 1 && g_live.empty());
    CHECK(five_owners(5) == 1 && g_live.empty());
    CHECK(five_owners(0) == 0 && g_live.empty());
    g_fail_at = 0;

    // h_pin / h_out 1 MiB, h_master / h_red 64 KiB, the index-list ring 4096, the fused pair list 2048 Int32, the pair buffers 64 entries
    const size_t floors[] = {(size_t)1 << 20, (size_t)1 << 16, 4096, 4 * 2048, 64};
    for (size_t f : floors) {
        const size_t needs[] = {1, f - 1, f, f + 1, 3 * f};
        const size_t want[] = {f, f, f, 2 * f, 4 * f};
        for (int i = 0; i < 5; ++i) {
            CHECK(grow_capacity(needs[i], f) == want[i]);
            CHECK(grow_capacity(needs[i], f) == old_capacity(needs[i], f));
            CHECK(grow_capacity(needs[i], 0) == needs[i]);      // no floor: exactly what is needed
        }
    }

    CHECK(g_live.empty() && g_allocs == g_frees);
    if (g_bad) { std::fprintf(stderr, "dev_mem_check: %d check(s) failed\n", g_bad); return 1; }
    std::printf("dev_mem_check ok: %ld allocations, %ld frees\n", g_allocs, g_frees);
    return 0;
}
