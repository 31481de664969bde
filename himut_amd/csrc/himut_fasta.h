// k_fasta_tricounts: reflib.get_chrom_tricount (reflib.py:11-33) over FASTA text as the file holds it.
//
// The input is the bytes of one record's sequence lines, line ends included.  The sequence is what is left after
// deleting '\n', '\r', '\t' and ' ' (the bytes read_fasta deletes); every other byte is a letter.  A triplet counts
// when its three letters are upper-case A/C/G/T; a purine centre is read on the other strand.  64 bins indexed
// first * 16 + centre * 4 + last with A0 C1 G2 T3 (only the 32 pyrimidine-centred ones fill).  A string that is
// already resident (himut_set_reference) is FASTA text without whitespace, so the same kernel counts it.
//
// One workgroup per tile of 4096 bytes (16 a lane, one 16-byte load), tiles grid-strided.  A triplet may straddle
// lanes, tiles and whitespace runs of any length, so every lane needs the first two letters behind its 16 bytes:
//   * each lane folds its bytes into a Follow (the first two letters of the bytes, 0, 1 or 2 of them);
//   * a suffix scan over the lanes (shuffles in the wave, then the later waves' totals through LDS) gives each
//     lane the Follow of everything behind it in the tile;
//   * wave 0 finds the tile's own followers by scanning forward past the tile end, 64 bytes a step, up to n;
//   * past n the caller's `tail` (the followers of the window end, found by the host) takes over.
// Histogram: a sub-histogram of the 32 pyrimidine-centred bins per wave in LDS, flushed once per workgroup.
//
// himut_strands.h includes this file for the substitution's class rule alone (sbs_bin; HIMUT_FASTA_NO_KERNELS): the
// kernels belong to himut_mut.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace himut {

constexpr int FASTA_TILE = 4096;              // bytes per workgroup tile (256 lanes x 16 B)

// byte -> 0..3 A/C/G/T, 4 any other letter (breaks triplets), 5 whitespace read_fasta deletes
__device__ __forceinline__ int fasta_code(int c) {
    switch (c) {
        case 'A': return 0;
        case 'C': return 1;
        case 'G': return 2;
        case 'T': return 3;
        case '\n': case '\r': case '\t': case ' ': return 5;
        default: return 4;
    }
}

// The first two letters of a byte range, packed: bits 0-1 how many (0..2), bits 2-4 the first code, bits 5-7 the second.
__host__ __device__ __forceinline__ uint32_t follow_push(uint32_t f, int code) {      // f, then one more letter
    const uint32_t cnt = f & 3;
    if (cnt == 0) return 1u | ((uint32_t)code << 2);
    if (cnt == 1) return 2u | (f & 0x1cu) | ((uint32_t)code << 5);
    return f;
}
__host__ __device__ __forceinline__ uint32_t follow_cat(uint32_t a, uint32_t b) {     // range a, then range b
    const uint32_t ca = a & 3;
    if (ca == 2 || (b & 3) == 0) return a;
    if (ca == 0) return b;
    return follow_push(a, (int)((b >> 2) & 7));
}

#ifndef HIMUT_FASTA_NO_KERNELS
__global__ void __launch_bounds__(256) k_fasta_tricounts(const uint8_t* p, int64_t n, uint32_t tail, unsigned long long* out) {
    __shared__ unsigned int s_h[4][32];
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_tail;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid < 128) s_h[tid >> 5][tid & 31] = 0;
    const int64_t ntiles = (n + FASTA_TILE - 1) / FASTA_TILE;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t t0 = t * FASTA_TILE, b0 = t0 + (int64_t)tid * 16;
        // this lane's 16 bytes (bytes at or past n are whitespace: they are not there)
        uint8_t by[16];
        if (b0 + 16 <= n) {
            const uint4 v = *reinterpret_cast<const uint4*>(p + b0);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 16; k++) by[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++) by[k] = b0 + k < n ? p[b0 + k] : (uint8_t)' ';
        }
        int code[16];
        uint32_t mine = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            code[k] = fasta_code(by[k]);
            if (code[k] != 5) mine = follow_push(mine, code[k]);
        }
        // wave 0: the tile's followers, scanning past the tile end (a whitespace run may be longer than a tile)
        if (wv == 0) {
            uint32_t f = 0;
            for (int64_t j = t0 + FASTA_TILE; (f & 3) < 2 && j < n; j += 64) {
                const int c = j + lane < n ? fasta_code(p[j + lane]) : 5;
                uint64_t m = __ballot(c != 5);
                while (m && (f & 3) < 2) {
                    const int src = __ffsll((unsigned long long)m) - 1;
                    f = follow_push(f, __shfl(c, src));
                    m &= m - 1;
                }
            }
            if (lane == 0) s_tail = follow_cat(f, tail);
        }
        // inclusive suffix scan of the lanes' Follows within the wave
        uint32_t inc = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_down(inc, d);
            if (lane + d < 64) inc = follow_cat(inc, o);
        }
        if (lane == 0) s_wave[wv] = inc;
        __syncthreads();
        uint32_t after = s_tail;                         // the later waves' totals, then the tile's followers
        for (int w = 3; w > wv; w--) after = follow_cat(s_wave[w], after);
        const uint32_t nxt = __shfl_down(inc, 1);
        const uint32_t fol = lane < 63 ? follow_cat(nxt, after) : after;
        int n1 = (fol & 3) >= 1 ? (int)((fol >> 2) & 7) : 4;
        int n2 = (fol & 3) >= 2 ? (int)((fol >> 5) & 7) : 4;
#pragma unroll
        for (int k = 15; k >= 0; k--) {
            const int a = code[k];
            if (a == 5) continue;
            if (a < 4 && n1 < 4 && n2 < 4) {
                const bool pur = n1 == 0 || n1 == 2;     // A or G in the middle: read the other strand
                const int f = pur ? 3 - n2 : a, m = pur ? 3 - n1 : n1, l = pur ? 3 - a : n2;
                atomicAdd(&s_h[wv][f * 8 + (m == 3 ? 4 : 0) + l], 1u);
            }
            n2 = n1;
            n1 = a;
        }
        __syncthreads();                                 // s_wave / s_tail are rewritten by the next tile
    }
    __syncthreads();
    if (tid < 32) {
        const unsigned int s = s_h[0][tid] + s_h[1][tid] + s_h[2][tid] + s_h[3][tid];
        const int f = tid >> 3, m = (tid & 4) ? 3 : 1, l = tid & 3;
        if (s) atomicAdd(&out[f * 16 + m * 4 + l], (unsigned long long)s);
    }
}
#endif  // HIMUT_FASTA_NO_KERNELS

// ---------------------------------------------------------------------------------------
// k_sbs<R>: mutlib.get_sbs96 (R = 1) / get_sbs1536 (R = 2) + the counting of load_sbs96_counts / load_sbs1536_counts
// (mutlib.py:1998-2055, 2058-2149) over the resident reference string: one thread per called single-base substitution
// (0-based position, ASCII ref / alt as the VCF holds them).  A purine reference base is reported on the other strand,
// its context through the purine2pyrimidine table (anything outside ACGTN becomes N); a pyrimidine one takes its
// context as the string holds it.  out[0 .. 6 * 4^2R - 1]: class (substitution C>A C>G C>T T>A T>C T>G), then the
// context letters from the farthest upstream to the farthest downstream, base 4 with A0 C1 G2 T3 (sbs96_lst /
// sbs1536_lst order); then three flags: classes that contain an N (the reference drops them); classes outside the list
// with no N (KeyError in the reference: a lower-case neighbour of a pyrimidine, an alt outside ACGT); position + R
// behind the string (IndexError).  A read below position 0 wraps to the END of the string, as python's seq[-1] does.
template <int R>
struct SbsBins {
    static constexpr int classes = 6 << (4 * R);          // 96, 1536
    static constexpr int total = classes + 3;
};

// the bin of one substitution: 0 .. classes - 1, or classes + 0 / 1 / 2 for the three flags (shared with k_sbs384,
// himut_strands.h)
template <int R>
__device__ __forceinline__ int sbs_bin(const uint8_t* seq, int64_t len, int64_t p, int r, int a) {
    constexpr int NC = SbsBins<R>::classes;
    auto code = [](int c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : c == 'N' ? 4 : 5; };   // 5: any other byte
    auto comp = [&](int c) { const int k = code(c); return k < 4 ? 3 - k : 4; };     // purine2pyrimidine.get(c, "N")
    if (p < 0 || p + R >= len) return NC + 2;
    const bool pur = r == 'A' || r == 'G';
    int up[R], dn[R];           // [k]: k + 1 places away; codes 0..3, 4 = N, 5 = a letter the class list does not have
    bool anyN = false, bad = false;
#pragma unroll
    for (int k = 0; k < R; k++) {
        const int64_t q = p - 1 - k;
        const int before = seq[q >= 0 ? q : q + len], after = seq[p + 1 + k];
        up[k] = pur ? comp(after) : code(before);
        dn[k] = pur ? comp(before) : code(after);
        anyN |= up[k] == 4 || dn[k] == 4;
        bad |= up[k] > 3 || dn[k] > 3;
    }
    const int rf = pur ? comp(r) : code(r), al = pur ? comp(a) : code(a);
    if (anyN || rf == 4 || al == 4) return NC;
    if (bad || al > 3 || (rf != 1 && rf != 3) || al == rf) return NC + 1;
    int idx = (rf == 1 ? 0 : 3) + (al > rf ? al - 1 : al);       // C>A C>G C>T | T>A T>C T>G
#pragma unroll
    for (int k = R - 1; k >= 0; k--) idx = idx * 4 + up[k];
#pragma unroll
    for (int k = 0; k < R; k++) idx = idx * 4 + dn[k];
    return idx;
}

#ifndef HIMUT_FASTA_NO_KERNELS
template <int R>
__global__ void __launch_bounds__(256) k_sbs(const uint8_t* seq, int64_t len, const int32_t* pos, const uint8_t* ref,
                                             const uint8_t* alt, int64_t n, unsigned long long* out) {
    constexpr int NB = SbsBins<R>::total;
    __shared__ unsigned int s_h[NB];
    for (int k = threadIdx.x; k < NB; k += blockDim.x) s_h[k] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(&s_h[sbs_bin<R>(seq, len, pos[i], ref[i], alt[i])], 1u);
    __syncthreads();
    for (int k = threadIdx.x; k < NB; k += blockDim.x)
        if (s_h[k]) atomicAdd(&out[k], (unsigned long long)s_h[k]);
}
#endif  // HIMUT_FASTA_NO_KERNELS

}  // namespace himut
