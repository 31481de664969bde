// Device code of the transcription-strand spectrum (himut_set_strands, himut_sbs384_counts, himut_strand_tricounts,
// himut_strand_callable; no counterpart in the reference).
//
// Genes reach the device as a segment list: start[k] ascending from 0, segment k covering [start[k], start[k + 1]) and the
// last one running to the string's end; mask[k] bit 0 = a gene on '+' covers the segment, bit 1 = a gene on '-' does.
// A position's category comes from its segment's mask and from whether the letter at the position (the VCF's REF, the
// trinucleotide's centre) is a purine, that is, whether k_sbs / k_fasta_tricounts read it on the other strand:
//     mask 0: N (3)    mask 1: pyrimidine U (1), purine T (0)    mask 2: pyrimidine T (0), purine U (1)    mask 3: B (2)
// T: the pyrimidine of the pair lies on the transcribed strand (SigProfiler's convention).  Order T, U, B, N.
//
//   k_sbs384             one thread per substitution, k_sbs<1>'s shape and its class rule (sbs_bin<1>, himut_fasta.h):
//                        bin = category * 96 + that bin; the three flags follow at 384..386 and have no category.
//   k_strand_tricounts   the resident string in tiles of 4096 positions, 16 bytes a lane in one load, tiles grid-strided.
//                        A lane's outer neighbours come from the lanes beside it by shuffle, a wave's from the waves
//                        beside it through LDS, the tile's two from the string (bounds-checked).  The tile's range of
//                        segments is found once per wave with wave-uniform searches (scalar registers); a lane searches
//                        that range for the segment of its first position and steps forward as it crosses starts.
//                        128 bins (category * 32 + class) per wave in LDS, one 64-bit atomicAdd per non-zero bin at the end.
//   k_strand_callable    the same tally over the CALLABLE entries of the callable run's map, eight entries a thread in one
//                        aligned load of the states (and one of the bases when a state is CALLABLE), an entry's position
//                        by IvGeo's geometry (himut_intervals.h): positions and bases, 128 bins each.
// The trinucleotide class is himut_run_intervals' (iv_class): first * 8 + (centre == T ? 4 : 0) + last after the fold; it
// exists only when all three letters are upper-case ACGT, so a position at either end of the string has none.
#pragma once

#include "himut_device.h"
#define HIMUT_FASTA_NO_KERNELS
#include "himut_fasta.h"
#define HIMUT_INTERVALS_NO_KERNELS
#include "himut_intervals.h"

namespace himut {

constexpr int ST_TILE = 4096, ST_BINS = 128, SBS384_BINS = 387;

struct StrandSegs {
    const int32_t* start;
    const uint8_t* mask;
    int64_t n;
};

__device__ __forceinline__ int strand_cat(int mask, bool purine) {
    return mask == 0 ? 3 : mask == 3 ? 2 : ((mask == 1) == purine ? 0 : 1);
}

// the first k in [lo, hi) with start[k] > p (hi when none)
__device__ __forceinline__ int64_t seg_upper(const int32_t* start, int64_t lo, int64_t hi, int64_t p) {
    while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (p < (int64_t)start[m]) hi = m; else lo = m + 1; }
    return lo;
}

// A lane's place in the segment list: segment k with mask m, the next start (none: past every position).
struct SegCursor {
    int64_t k, next;
    int m;
    __device__ __forceinline__ void at(const StrandSegs& S, int64_t k_) {
        k = k_; m = S.mask[k]; next = k + 1 < S.n ? (int64_t)S.start[k + 1] : INT64_MAX;
    }
    __device__ __forceinline__ void seek(const StrandSegs& S, int64_t lo, int64_t hi, int64_t p) { at(S, seg_upper(S.start, lo, hi, p) - 1); }
};

// the class of three letter codes (iv_code: 0..3, -1 any other byte): 0..31, IV_OTHER without one
__device__ __forceinline__ int tri_class_codes(int a, int m, int b) {
    if ((a | m | b) < 0) return IV_OTHER;
    if (m & 1) return a * 8 + (m == 3 ? 4 : 0) + b;
    return (3 - b) * 8 + (m == 0 ? 4 : 0) + (3 - a);
}

__global__ void __launch_bounds__(256) k_sbs384(const uint8_t* seq, int64_t len, StrandSegs S, const int32_t* pos, const uint8_t* ref,
                                                const uint8_t* alt, int64_t n, uint16_t* cls, unsigned long long* out) {
    __shared__ unsigned int s_h[SBS384_BINS];
    for (int k = threadIdx.x; k < SBS384_BINS; k += blockDim.x) s_h[k] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = pos[i];
        const int r = ref[i];
        const int64_t k = p >= 0 && p < len ? seg_upper(S.start, (int64_t)1, S.n, p) - 1 : 0;
        const int b = sbs_bin<1>(seq, len, p, r, alt[i]);
        const int bin = b >= 96 ? 384 + (b - 96) : strand_cat(S.mask[k], r == 'A' || r == 'G') * 96 + b;
        atomicAdd(&s_h[bin], 1u);
        if (cls) cls[i] = b >= 96 ? (uint16_t)0xFFFFu : (uint16_t)bin;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < SBS384_BINS; k += blockDim.x)
        if (s_h[k]) atomicAdd(&out[k], (unsigned long long)s_h[k]);
}

__global__ void __launch_bounds__(256) k_strand_tricounts(const uint8_t* p, int64_t n, StrandSegs S, unsigned long long* out) {
    __shared__ unsigned int s_h[4][ST_BINS];
    __shared__ int s_first[2][4], s_last[2][4];          // a wave's first and last letter codes, two tiles in flight
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int k = tid; k < 4 * ST_BINS; k += 256) (&s_h[0][0])[k] = 0;
    const int64_t ntiles = (n + ST_TILE - 1) / ST_TILE;
    int par = 0;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x, par ^= 1) {
        const int64_t t0 = t * ST_TILE, b0 = t0 + (int64_t)tid * 16, tend = min(t0 + ST_TILE, n);
        // this lane's 16 letters as codes (positions at or past n: no letter)
        int code[16];
        if (b0 + 16 <= n) {
            const uint4 v = *reinterpret_cast<const uint4*>(p + b0);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 16; k++) code[k] = iv_code((int)((w[k >> 2] >> (8 * (k & 3))) & 0xffu));
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++) code[k] = b0 + k < n ? iv_code(p[b0 + k]) : -1;
        }
        // the tile's two halo letters, from the string
        int halo = -1;
        if (tid == 0 && t0 > 0) halo = iv_code(p[t0 - 1]);
        if (tid == 255 && t0 + ST_TILE < n) halo = iv_code(p[t0 + ST_TILE]);
        if (lane == 0) s_first[par][wv] = code[0];
        if (lane == 63) s_last[par][wv] = code[15];
        // the tile's segments [k_lo, k_hi): wave-uniform
        const int64_t k_lo = uni(seg_upper(S.start, (int64_t)1, S.n, t0) - 1);
        const int64_t k_hi = uni(seg_upper(S.start, k_lo + 1, S.n, tend - 1));
        __syncthreads();        // (one barrier a tile: the next tile writes the other half of s_first / s_last)
        int left = __shfl_up(code[15], 1), right = __shfl_down(code[0], 1);
        if (lane == 0) left = wv > 0 ? s_last[par][wv - 1] : halo;
        if (lane == 63) right = wv < 3 ? s_first[par][wv + 1] : halo;
        if (b0 < tend) {
            SegCursor c;
            c.seek(S, k_lo + 1, k_hi, b0);
            int prev = left;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const int64_t q = b0 + j;
                while (q >= c.next) c.at(S, c.k + 1);
                const int cl = tri_class_codes(prev, code[j], j < 15 ? code[j + 1] : right);
                if (cl < IV_OTHER) atomicAdd(&s_h[wv][strand_cat(c.m, !(code[j] & 1)) * 32 + cl], 1u);
                prev = code[j];
            }
        }
    }
    __syncthreads();
    if (tid < ST_BINS) {
        const unsigned long long s = (unsigned long long)s_h[0][tid] + s_h[1][tid] + s_h[2][tid] + s_h[3][tid];
        if (s) atomicAdd(&out[tid], s);
    }
}

// out[0..127]: positions, out[128..255]: bases.  N: the map's entries.
__global__ void __launch_bounds__(256) k_strand_callable(IvGeo G, StrandSegs S, int64_t N, unsigned long long* out) {
    __shared__ unsigned long long s_h[2 * ST_BINS];
    const int tid = threadIdx.x;
    s_h[tid] = 0;
    __syncthreads();
    const int64_t ngroups = (N + IV_PER - 1) / IV_PER;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + tid; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i0 = g * IV_PER;
        // (both arrays carry a block of slack behind the map's last entry: aligned loads inside the buffers)
        const uint2 sv = *reinterpret_cast<const uint2*>(G.mstate + i0);
        const uint64_t s8 = (uint64_t)sv.x | ((uint64_t)sv.y << 32);
        bool any = false;
#pragma unroll
        for (int k = 0; k < IV_PER; k++) any |= i0 + k < N && ((s8 >> (8 * k)) & 0xffu) == (uint64_t)HIMUT_CM_CALLABLE;
        if (!any) continue;
        const uint4 bv = *reinterpret_cast<const uint4*>(G.mbases + i0);
        const uint32_t bw[4] = {bv.x, bv.y, bv.z, bv.w};
        int64_t c = upper_bound(G.mapoff, (int64_t)0, G.nch + 1, i0) - 1;      // the chunk of entry i0
        int64_t next = G.mapoff[c + 1];
        SegCursor sc;
        int64_t seg_lo = 0;
        sc.k = -1; sc.next = 0; sc.m = 0;                                     // (no segment yet)
#pragma unroll
        for (int k = 0; k < IV_PER; k++) {
            const int64_t m = i0 + k;
            if (m >= N || ((s8 >> (8 * k)) & 0xffu) != (uint64_t)HIMUT_CM_CALLABLE) continue;
            while (m >= next) { c++; next = G.mapoff[c + 1]; }                 // (chunks without a position are stepped over)
            const int64_t rpos = (int64_t)G.cs[c] + (m - G.mapoff[c]);
            if (rpos < 1 || rpos + 2 > G.reflen) continue;
            const int mid = iv_code(G.refseq[rpos]);
            const int cl = tri_class_codes(iv_code(G.refseq[rpos - 1]), mid, iv_code(G.refseq[rpos + 1]));
            if (cl >= IV_OTHER) continue;
            if (sc.k < 0 || rpos < seg_lo || rpos >= sc.next) {               // another segment (chunks may overlap or go back)
                sc.seek(S, (int64_t)1, S.n, rpos);
                seg_lo = S.start[sc.k];
            }
            const int bin = strand_cat(sc.m, !(mid & 1)) * 32 + cl;
            atomicAdd(&s_h[bin], 1ull);
            atomicAdd(&s_h[ST_BINS + bin], (unsigned long long)((bw[k >> 1] >> (16 * (k & 1))) & 0xffffu));
        }
    }
    __syncthreads();
    if (s_h[tid]) atomicAdd(&out[tid], s_h[tid]);
}

}  // namespace himut
