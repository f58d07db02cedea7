// Microbenchmark: the memory floor of the per-step counting sort's two big launches, at n = 1e7 and n = 1.25e6.
//   leg (a)  the histogram's traffic: one pass over 4 B x n (bins) + 2 B x n (prev_lab), 16-byte loads per lane
//   leg (b)  the scatter's traffic: read 4 B x n, write 4 B x n to the positions of a real stable counting sort by bin = (label, sub-label),
//            K = 32: points of a component contiguous in storage with the two sub-labels mixed (the bench data: long runs per bin), and
//            labels in no particular storage order (every 64 consecutive points go to ~40 different places)
// Both legs as one wave per 2048-point tile / 512-point tile (the sort's launch shapes) and as 256-thread workgroups, four tiles each.
//   hipcc --offload-arch=gfx950 -O3 scripts/microbench/sort_floor.hip -o scripts/microbench/sort_floor.bin
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>

template <int TILE, int W>
__global__ __launch_bounds__(64 * W) void read_leg(const int4 *__restrict__ bins, const uint2 *__restrict__ prev, int *__restrict__ out, int nt) {
    const int tile = blockIdx.x * W + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tile >= nt) return;
    const int4 *p = bins + (size_t)tile * (TILE / 4);
    const int4 *q = reinterpret_cast<const int4 *>(prev + (size_t)tile * (TILE / 4));        // (eight 16-bit labels per 16-byte load)
    int4 v[TILE / 256], u[TILE / 512];
#pragma unroll
    for (int i = 0; i < TILE / 256; ++i) v[i] = p[i * 64 + lane];
#pragma unroll
    for (int i = 0; i < TILE / 512; ++i) u[i] = q[i * 64 + lane];
    int s = 0;
#pragma unroll
    for (int i = 0; i < TILE / 256; ++i) s += v[i].x + v[i].y + v[i].z + v[i].w;
#pragma unroll
    for (int i = 0; i < TILE / 512; ++i) s += u[i].x + u[i].y + u[i].z + u[i].w;
    if (s == 123456789) out[tile] = s;
}

template <int TILE, int W>
__global__ __launch_bounds__(64 * W) void scatter_leg(const int4 *__restrict__ pos, int *__restrict__ perm, int nt) {
    const int tile = blockIdx.x * W + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tile >= nt) return;
    const int4 *p = pos + (size_t)tile * (TILE / 4);
    int4 v[TILE / 256];
#pragma unroll
    for (int i = 0; i < TILE / 256; ++i) v[i] = p[i * 64 + lane];
#pragma unroll
    for (int i = 0; i < TILE / 256; ++i) {
        const int i0 = tile * TILE + (i * 64 + lane) * 4;
        perm[v[i].x] = i0; perm[v[i].y] = i0 + 1; perm[v[i].z] = i0 + 2; perm[v[i].w] = i0 + 3;
    }
}

static uint32_t mix(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }

int main() {
    const int K = 32, nbins = 2 * K;
    for (size_t n : {(size_t)10000000, (size_t)1250000}) {
        const size_t npad = (n + 2047) / 2048 * 2048;
        int *bins, *pos, *perm, *out; uint16_t *prev;
        hipMalloc(&bins, npad * 4); hipMalloc(&pos, npad * 4); hipMalloc(&perm, npad * 4); hipMalloc(&prev, npad * 2); hipMalloc(&out, npad / 512 * 4 + 64);
        hipMemset(bins, 1, npad * 4); hipMemset(prev, 1, npad * 2);
        hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
        auto timeit = [&](const char *name, double bytes, auto launch) {
            for (int i = 0; i < 3; ++i) launch();
            hipEventRecord(a);
            for (int i = 0; i < 20; ++i) launch();
            hipEventRecord(b); hipEventSynchronize(b);
            float ms; hipEventElapsedTime(&ms, a, b);
            printf("n=%-9zu %-58s %7.2f us  %5.2f TB/s\n", n, name, 1e3 * ms / 20, bytes / (ms / 20 * 1e-3) / 1e12);
        };
        const int nt2048 = (int)(npad / 2048), nt512 = (int)(npad / 512);
        timeit("(a) read 4B+2B, one wave per 2048-point tile", 6.0 * n, [&] { hipLaunchKernelGGL((read_leg<2048, 1>), dim3(nt2048), dim3(64), 0, 0, (const int4 *)bins, (const uint2 *)prev, out, nt2048); });
        timeit("(a) read 4B+2B, 8 x 2048-point tiles per workgroup", 6.0 * n, [&] { hipLaunchKernelGGL((read_leg<2048, 8>), dim3((nt2048 + 7) / 8), dim3(512), 0, 0, (const int4 *)bins, (const uint2 *)prev, out, nt2048); });
        timeit("(a) read 4B+2B, 4 x 512-point tiles per workgroup", 6.0 * n, [&] { hipLaunchKernelGGL((read_leg<512, 4>), dim3((nt512 + 3) / 4), dim3(256), 0, 0, (const int4 *)bins, (const uint2 *)prev, out, nt512); });
        timeit("(a) read 4B+2B, 8 x 512-point tiles per workgroup", 6.0 * n, [&] { hipLaunchKernelGGL((read_leg<512, 8>), dim3((nt512 + 7) / 8), dim3(512), 0, 0, (const int4 *)bins, (const uint2 *)prev, out, nt512); });
        for (int shuffled = 0; shuffled < 2; ++shuffled) {
            // the destination of every point under a stable counting sort by bin (padding points keep their own place)
            std::vector<int> hb(npad), hp(npad);
            std::vector<size_t> cnt(nbins + 1, 0);
            for (size_t i = 0; i < n; ++i) {
                const uint32_t r = mix((uint32_t)i * 2654435761u + 12345u);
                const int k = shuffled ? (int)((r >> 8) % K) : (int)(i * K / n);
                hb[i] = 2 * k + (int)(r & 1u);
                ++cnt[hb[i] + 1];
            }
            for (int bq = 0; bq < nbins; ++bq) cnt[bq + 1] += cnt[bq];
            for (size_t i = 0; i < n; ++i) hp[i] = (int)cnt[hb[i]]++;
            for (size_t i = n; i < npad; ++i) hp[i] = (int)i;
            hipMemcpy(pos, hp.data(), npad * 4, hipMemcpyHostToDevice);
            char nm[96];
            snprintf(nm, 96, "(b) %s: one wave per 2048-point tile", shuffled ? "shuffled" : "contiguous");
            timeit(nm, 8.0 * n, [&] { hipLaunchKernelGGL((scatter_leg<2048, 1>), dim3(nt2048), dim3(64), 0, 0, (const int4 *)pos, perm, nt2048); });
            snprintf(nm, 96, "(b) %s: 4 x 2048-point tiles per workgroup", shuffled ? "shuffled" : "contiguous");
            timeit(nm, 8.0 * n, [&] { hipLaunchKernelGGL((scatter_leg<2048, 4>), dim3((nt2048 + 3) / 4), dim3(256), 0, 0, (const int4 *)pos, perm, nt2048); });
            snprintf(nm, 96, "(b) %s: 4 x 512-point tiles per workgroup", shuffled ? "shuffled" : "contiguous");
            timeit(nm, 8.0 * n, [&] { hipLaunchKernelGGL((scatter_leg<512, 4>), dim3((nt512 + 3) / 4), dim3(256), 0, 0, (const int4 *)pos, perm, nt512); });
            snprintf(nm, 96, "(b) %s: one wave per 512-point tile", shuffled ? "shuffled" : "contiguous");
            timeit(nm, 8.0 * n, [&] { hipLaunchKernelGGL((scatter_leg<512, 1>), dim3(nt512), dim3(64), 0, 0, (const int4 *)pos, perm, nt512); });
        }
        hipFree(bins); hipFree(pos); hipFree(perm); hipFree(prev); hipFree(out);
    }
    return 0;
}
