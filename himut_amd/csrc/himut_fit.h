// k_fit_resample, k_fit_em: signature exposures of a spectrum with bootstrap replicates (include/himut_hip.h,
// himut_fit_exposures).  No counterpart in the reference.  The definition is this package's
// and is written out in the header; what matters here is the order of the sums, which is the specification:
//
//   step 1, per channel c:    r[c] = sum over k of S[c][k] * e[k], ascending k from 0.0;  q[c] = m[c] / r[c], or 0.0 when
//                             m[c] == 0 or r[c] == 0.0
//   step 2, per signature k:  g = sum over c of S[c][k] * q[c], ascending c from 0.0;  e[k] = e[k] * g
//
// One multiply and one add per term (__dmul_rn / __dadd_rn: nothing contracts them, whatever the build's flags), the
// division is the compiler's correctly rounded fp64 sequence.  A lane per channel in step 1 and a lane per signature in
// step 2 give exactly those orders; no sum is split across lanes.
//
// Layout.  A replicate is fitted by one wave: its lanes stride the channels in step 1 and the signatures in step 2, its
// counts m, quotients q and exposures e live in LDS.  Step 2 is K (<= 96) chains of C dependent adds, so a wider team
// would only idle; instead up to FIT_WAVES waves, a replicate each, share a workgroup and with it the one copy of S in
// LDS.  S rows are padded to an odd number of doubles there: in step 1 the lanes of a wave read one column of 64
// consecutive rows, and an odd row stride spreads them over all banks (an even one such as K = 30 folds them onto 16).
// The host keeps S in LDS whenever it fits the workgroup's LDS budget beside one replicate's arrays and gives up replicates
// per workgroup first (measured: S in LDS is worth 1.7 x at 96 x 30, the replicates per workgroup nothing).  Where it does
// not fit, S is read from global memory as the host laid it out ([C][K], unpadded): every replicate reads the same
// C * K * 8 bytes, which stay in L2.  Workgroups stride
// over the replicates when there are more than the grid holds.
//
// k_fit_resample draws replicates 1..B (replicate 0 is the spectrum itself): a workgroup owns a replicate, holds the
// inclusive prefix sums of m and the replicate's histogram in LDS, its threads stride the N draws, each a splitmix64
// value of (seed, b, i) and a binary search of the prefix sums; the histogram is written once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace himut {

constexpr int FIT_MAX_C = 1536, FIT_MAX_K = 96;
constexpr int FIT_MAX_BOOT = 100000, FIT_MAX_ITERS = 100000;
constexpr int FIT_WAVES = 4;                        // the most replicates that share a workgroup of k_fit_em (a wave each)
constexpr int FIT_LDS_BUDGET = 64 * 1024;           // bytes of LDS a workgroup of k_fit_em may take (himut_debug_fit)

// doubles of a row of S in LDS: K rounded up to odd
__host__ __device__ inline int fit_row_stride(int K) { return K | 1; }
// bytes of LDS one replicate takes beside S: q[C] and e[K] as doubles, m[C] as int32
__host__ __device__ inline size_t fit_rep_bytes(int C, int K) { return (size_t)C * 8 + (size_t)K * 8 + (size_t)C * 4; }

// draw i of replicate b: splitmix64 of seed + golden * (1 + b * 2^32 + i), the high word scaled to 0..N-1
__host__ __device__ inline uint32_t fit_draw(uint64_t seed, uint64_t b, uint64_t i, uint32_t N) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (1ull + (b << 32) + i);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)(((z >> 32) * (uint64_t)N) >> 32);
}

// counts: m[C]; prefix: its inclusive prefix sums (the last one is N < 2^31); out[(B + 1)][C]: row 0 = m, row b = the
// histogram of replicate b's N draws.  Dynamic LDS: 2 * C words.
__global__ void __launch_bounds__(256) k_fit_resample(const int32_t* __restrict__ counts, const uint32_t* __restrict__ prefix,
                                                      int C, uint32_t N, int n_boot, uint64_t seed, int32_t* __restrict__ out) {
    extern __shared__ uint32_t fit_words[];
    uint32_t* s_pre = fit_words;
    uint32_t* s_h = fit_words + C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) s_pre[c] = prefix[c];
    for (int b = blockIdx.x; b <= n_boot; b += gridDim.x) {
        if (b == 0) {
            for (int c = threadIdx.x; c < C; c += blockDim.x) out[c] = counts[c];
            continue;
        }
        for (int c = threadIdx.x; c < C; c += blockDim.x) s_h[c] = 0;
        __syncthreads();                            // the prefix sums (first pass) and the zeros are in place
        for (uint32_t i = threadIdx.x; i < N; i += blockDim.x) {
            const uint32_t j = fit_draw(seed, (uint64_t)b, i, N);
            int lo = 0, hi = C - 1;                 // the smallest c with s_pre[c] > j: s_pre[C - 1] = N > j
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_pre[mid] > j) hi = mid; else lo = mid + 1;
            }
            atomicAdd(&s_h[lo], 1u);
        }
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += blockDim.x) out[(size_t)b * C + c] = (int32_t)s_h[c];
        __syncthreads();                            // before the next replicate clears the histogram
    }
}

// sig[C][K] row-major; counts[n_rep][C] (k_fit_resample's out); e0 = (double)N / (double)K; expo[n_rep][K].  blockDim =
// 64 * waves, a replicate per wave.  Dynamic LDS, doubles first: with S_IN_LDS the C rows of S at fit_row_stride(K), then
// per wave q[C] and e[K], then per wave m[C] as int32.
template <bool S_IN_LDS>
__global__ void __launch_bounds__(64 * FIT_WAVES) k_fit_em(const double* __restrict__ sig, int C, int K,
                                                           const int32_t* __restrict__ counts, int n_rep, double e0, int iters,
                                                           double* __restrict__ expo) {
    extern __shared__ double fit_lds[];
    const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int stride = S_IN_LDS ? fit_row_stride(K) : K;
    double* s_sig = fit_lds;
    double* s_q = fit_lds + (S_IN_LDS ? (size_t)C * stride : 0) + (size_t)wave * (C + K);
    double* s_e = s_q + C;
    int32_t* s_m = reinterpret_cast<int32_t*>(fit_lds + (S_IN_LDS ? (size_t)C * stride : 0) + (size_t)waves * (C + K)) + (size_t)wave * C;
    if (S_IN_LDS)
        for (int i = threadIdx.x; i < C * K; i += blockDim.x) s_sig[(i / K) * stride + i % K] = sig[i];
    const double* S = S_IN_LDS ? s_sig : sig;
    // every wave of the workgroup makes the same trips and meets the same barriers; one without a replicate only waits
    for (int base = blockIdx.x * waves; base < n_rep; base += gridDim.x * waves) {
        const int rep = base + wave;
        const bool live = rep < n_rep;
        if (live) {
            for (int c = lane; c < C; c += 64) s_m[c] = counts[(size_t)rep * C + c];
            for (int k = lane; k < K; k += 64) s_e[k] = e0;
        }
        __syncthreads();
        for (int t = 0; t < iters; t++) {
            if (live)
                for (int c = lane; c < C; c += 64) {
                    const double* row = S + (size_t)c * stride;
                    double r = 0.0;
                    for (int k = 0; k < K; k++) r = __dadd_rn(r, __dmul_rn(row[k], s_e[k]));
                    const int32_t m = s_m[c];
                    s_q[c] = (m == 0 || r == 0.0) ? 0.0 : (double)m / r;
                }
            __syncthreads();
            if (live)
                for (int k = lane; k < K; k += 64) {
                    const double* col = S + k;
                    double g = 0.0;
                    for (int c = 0; c < C; c++) g = __dadd_rn(g, __dmul_rn(col[(size_t)c * stride], s_q[c]));
                    s_e[k] = __dmul_rn(s_e[k], g);
                }
            __syncthreads();
        }
        if (live)
            for (int k = lane; k < K; k += 64) expo[(size_t)rep * K + k] = s_e[k];
    }
}

}  // namespace himut
