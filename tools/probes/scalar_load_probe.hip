// Probe: what ONE DEPENDENT scalar load (s_load_dword, waited for with s_waitcnt lgkmcnt(0) before the next can issue) costs a wave —
// the price of every kernel parameter that is fetched at its point of use (a field of MlmDev / MlmFrame behind MLM_SLOT_SETUP).
// A chain of HOPS loads walks a small table, every hop on a 64-byte line of its own: word 16 * k holds the byte offset of hop k + 1.
//   pass 0 is the first touch after the kernel start (the scalar cache is invalidated there: the lines come from L2; the pass also
//   fetches the loop's code),
//   passes 1 and 2 walk the same lines again (warm in the scalar cache).
// Every CU gets W workgroups of 256 threads (= W waves per SIMD; the LDS request keeps a (W+1)-th away), all waves walk the SAME
// table (as all workgroups of a launch read the same slot); min / median / max over the waves, in shader clocks (s_memtime).
// Build: hipcc --offload-arch=gfx950 -O3 -o scalar_load_probe scalar_load_probe.hip ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#define HOPS 32
#define PASSES 3
#define CONSTANT __attribute__((address_space(4)))

__device__ __forceinline__ uint32_t chase(const CONSTANT unsigned char *tab, uint32_t off) {
#pragma unroll
    for (int k = 0; k < HOPS; ++k) off = *(const CONSTANT uint32_t *)(tab + off); // uniform address, constant space: s_load_dword
    return off;
}

__global__ __launch_bounds__(256) void k_chain(const uint32_t *table, uint32_t *out, uint32_t n_waves) {
    extern __shared__ unsigned char pad[];
    if (n_waves == 0xFFFFFFFFu) pad[threadIdx.x] = 1; // (keeps the LDS request alive)
    const CONSTANT unsigned char *tab = (const CONSTANT unsigned char *)(unsigned long long)table;
    uint32_t off = 0;
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    const bool writer = (threadIdx.x & 63) == 0 && wave < n_waves;
#pragma unroll 1 // (every pass runs the SAME instructions: from the second pass on the code is in the instruction cache as well)
    for (int p = 0; p < PASSES; ++p) {
        const unsigned long long t0 = __builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(off)::"memory"); // (the chain starts behind the stamp ...)
        off = chase(tab, off);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(off)::"memory"); // (... and has ended in front of this one)
        const unsigned long long t1 = __builtin_amdgcn_s_memtime();
        if (writer) out[(size_t)p * n_waves + wave] = (uint32_t)(t1 - t0) + (off & 0u); // (the chain's end is 0 again: keeps it alive)
    }
}

// the two s_memtime reads and waits alone
__global__ __launch_bounds__(256) void k_empty(uint32_t *out, uint32_t n_waves) {
    unsigned long long dt = 0;
#pragma unroll 1 // (the second round's instructions are in the instruction cache: that one counts)
    for (int p = 0; p < 2; ++p) {
        const unsigned long long t0 = __builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        dt = __builtin_amdgcn_s_memtime() - t0;
    }
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0 && wave < n_waves) out[wave] = (uint32_t)dt;
}

static void stats(std::vector<uint32_t> v, double sub, double div, const char *what) {
    std::sort(v.begin(), v.end());
    printf("    %-34s min %7.1f  median %7.1f  p90 %7.1f  max %8.1f\n", what, (v.front() - sub) / div, (v[v.size() / 2] - sub) / div,
           (v[v.size() * 9 / 10] - sub) / div, (v.back() - sub) / div);
}

int main() {
    hipDeviceProp_t prop;
    hipGetDeviceProperties(&prop, 0);
    const int n_cu = prop.multiProcessorCount;
    printf("device %s, %d CUs; %d dependent s_load_dword per pass, one 64-byte line per hop; shader clocks per hop (two s_memtime reads taken off)\n",
           prop.name, n_cu, HOPS);
    // hop k -> line (7 k + 3) mod HOPS ... back to offset 0 after HOPS hops (a permutation: no next-line regularity)
    std::vector<uint32_t> h_tab(HOPS * 16, 0u);
    {
        uint32_t line = 0;
        std::vector<uint32_t> order;
        for (int k = 0; k < HOPS; ++k) order.push_back((uint32_t)((7 * k) % HOPS)); // 7 and 32 are coprime: every line once, line 0 first
        for (int k = 0; k < HOPS; ++k) {
            line = order[k];
            h_tab[line * 16] = order[(k + 1) % HOPS] * 64u;
        }
    }
    uint32_t *d_tab, *d_out;
    hipMalloc(&d_tab, h_tab.size() * 4);
    hipMemcpy(d_tab, h_tab.data(), h_tab.size() * 4, hipMemcpyHostToDevice);
    const uint32_t max_waves = (uint32_t)n_cu * 8u * 4u;
    hipMalloc(&d_out, (size_t)PASSES * max_waves * 4);
    for (int W : {1, 8}) {
        const uint32_t n_waves = (uint32_t)n_cu * (uint32_t)W * 4u;
        const size_t lds = (size_t)(160 * 1024 / W) - 1024; // W workgroups fill a CU's LDS: no (W+1)-th
        hipFuncSetAttribute((const void *)k_chain, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        std::vector<uint32_t> h(PASSES * (size_t)n_waves), e(n_waves);
        for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL(k_empty, dim3(n_waves / 4), dim3(256), 0, 0, d_out, n_waves); // (the first loads the code)
        hipMemcpy(e.data(), d_out, (size_t)n_waves * 4, hipMemcpyDeviceToHost);
        std::sort(e.begin(), e.end());
        const double base = (double)e[e.size() / 2];
        for (int rep = 0; rep < 3; ++rep) { // (rep 0 also loads the code and brings the table into L2)
            hipLaunchKernelGGL(k_chain, dim3(n_waves / 4), dim3(256), lds, 0, d_tab, d_out, n_waves);
            if (hipDeviceSynchronize() != hipSuccess) {
                printf("launch failed\n");
                return 1;
            }
            hipMemcpy(h.data(), d_out, h.size() * 4, hipMemcpyDeviceToHost);
            printf("%d wave(s) per SIMD (%u waves), launch %d; empty stamp pair: %.0f clocks\n", W, n_waves, rep, base);
            const char *names[PASSES] = {"first touch after the kernel start", "second pass (warm scalar cache)", "third pass (warm scalar cache)"};
            for (int p = 0; p < PASSES; ++p)
                stats(std::vector<uint32_t>(h.begin() + (size_t)p * n_waves, h.begin() + (size_t)(p + 1) * n_waves), base, (double)HOPS, names[p]);
        }
    }
    hipFree(d_tab);
    hipFree(d_out);
    return 0;
}
