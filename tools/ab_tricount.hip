// A/B of the trinucleotide count on a resident string (tools only): k_fasta_tricounts, the kernel the library uses
// for both the FASTA path and himut_ref_tricounts, against the per-position kernel it replaced (kept here, verbatim
// in its logic, as the baseline).  Same string, same call, alternating, 64 Mb and 3.1 Gb; counts must agree.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I himut_amd/csrc -o /tmp/ab_tricount tools/ab_tricount.hip && /tmp/ab_tricount
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "himut_fasta.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

// the previous kernel: one thread per position, three byte loads, one LDS histogram per workgroup
__global__ void __launch_bounds__(256) k_ref_tricounts_old(const uint8_t* seq, int64_t len, unsigned long long* out) {
    __shared__ unsigned int s_h[64];
    if (threadIdx.x < 64) s_h[threadIdx.x] = 0;
    __syncthreads();
    auto code = [](int c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; };
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i + 2 < len; i += (int64_t)gridDim.x * blockDim.x) {
        const int a = code(seq[i]), b = code(seq[i + 1]), d = code(seq[i + 2]);
        if (a > 3 || b > 3 || d > 3) continue;
        const bool pur = b == 0 || b == 2;
        const int f = pur ? 3 - d : a, m = pur ? 3 - b : b, l = pur ? 3 - a : d;
        atomicAdd(&s_h[f * 16 + m * 4 + l], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 64 && s_h[threadIdx.x]) atomicAdd(&out[threadIdx.x], (unsigned long long)s_h[threadIdx.x]);
}

// a genome-like string: mostly ACGT, soft-masked and N stretches (hash of the position, no host copy)
__global__ void k_fill(uint8_t* s, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t h = (uint64_t)i * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
        const uint64_t blk = ((uint64_t)(i >> 12) * 0x94D049BB133111EBull) >> 58;   // 4 kb stretches
        const char c = "ACGT"[h & 3];
        s[i] = blk == 0 ? 'N' : blk < 20 ? (uint8_t)(c + 32) : (uint8_t)c;
    }
}

int main() {
    const int64_t sizes[2] = {64ll << 20, 3100000000ll};
    for (int64_t n : sizes) {
        uint8_t* d = nullptr;
        unsigned long long* out = nullptr;
        CK(hipMalloc(&d, (size_t)n));
        CK(hipMalloc(&out, 2 * 64 * 8));
        hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, 0, d, n);
        CK(hipDeviceSynchronize());
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        std::vector<float> t_old, t_new;
        const int64_t tiles = (n + himut::FASTA_TILE - 1) / himut::FASTA_TILE;
        for (int rep = 0; rep < 11; rep++) {
            for (int which = 0; which < 2; which++) {
                CK(hipMemset(out + which * 64, 0, 64 * 8));
                CK(hipEventRecord(e0));
                if (which == 0) hipLaunchKernelGGL(k_ref_tricounts_old, dim3(2048), dim3(256), 0, 0, d, n, out);
                else hipLaunchKernelGGL(himut::k_fasta_tricounts, dim3((unsigned)std::min<int64_t>(tiles, 2048)), dim3(256), 0, 0, d, n, 0u, out + 64);
                CK(hipEventRecord(e1));
                CK(hipEventSynchronize(e1));
                float ms = 0;
                CK(hipEventElapsedTime(&ms, e0, e1));
                if (rep > 0) (which == 0 ? t_old : t_new).push_back(ms);     // rep 0 is the warm-up
            }
        }
        unsigned long long h[128];
        CK(hipMemcpy(h, out, sizeof(h), hipMemcpyDeviceToHost));
        bool same = true;
        unsigned long long tot = 0;
        for (int k = 0; k < 64; k++) { same &= h[k] == h[64 + k]; tot += h[k]; }
        std::sort(t_old.begin(), t_old.end());
        std::sort(t_new.begin(), t_new.end());
        const double mo = t_old[t_old.size() / 2], mn = t_new[t_new.size() / 2];
        printf("{\"bytes\": %lld, \"old_ms\": %.4f, \"new_ms\": %.4f, \"old_GBps\": %.1f, \"new_GBps\": %.1f, \"same_counts\": %s, \"triplets\": %llu}\n",
               (long long)n, mo, mn, n / mo / 1e6, n / mn / 1e6, same ? "true" : "false", tot);
        CK(hipFree(d)); CK(hipFree(out));
        CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
        if (!same) return 2;
    }
    return 0;
}
