// Device code of the intervals run (himut_run_intervals): the callable run's map (himut_callmap.h: a state byte and a
// 16-bit count of callable bases per swept position, the chunks one behind the other) tallied per interval -- entries
// and bases per state, and three histograms over the trinucleotide class of the position (the key rule of norm_tribins,
// himut_sweep.h, folded to 32 classes and "other").
//
//   k_iv_plan    a thread per interval: the map entries the interval holds and how many spans they make.  Chunks that
//                are ascending and disjoint (the host looked) lie in the map in position order, so an interval holds one
//                contiguous range of entries, found with two binary searches in the chunk bounds; otherwise the thread
//                walks every chunk and the interval holds a range per chunk it meets.
//                A span: at most IV_SPAN entries of one range, cut from the range's first entry rounded down to 8, so
//                that every thread's eight entries are one aligned load of the states and one of the bases; what lies in
//                front of the range or behind it is masked, not assumed away.
//   (rocPRIM's exclusive scan puts the spans of all intervals one behind the other)
//   k_iv_tally   a fixed grid; a workgroup takes an equal share of consecutive spans, finds its first span's interval with
//                one binary search and steps on from there.  Per span: 128 32-bit counters in LDS (IV_SPAN x 65,535 < 2^32),
//                256 threads x 8 entries at a time, then one 64-bit atomicAdd per non-zero counter into the interval's row.
//                Nothing waits for the host between the plan and the tally, and no list of spans is written: a span's
//                range is recomputed from its interval's (the slow path walks the chunks again for it).
// himut_strands.h includes this file for the geometry and the class rule alone (HIMUT_INTERVALS_NO_KERNELS): the kernels
// belong to himut_intervals.hip.
#pragma once

#include <cstddef>

#include "himut_device.h"

namespace himut {

constexpr int IV_NT = 256, IV_PER = 8, IV_SLICE = IV_NT * IV_PER, IV_SPAN_SLICES = 16, IV_CELLS = 128;
constexpr int64_t IV_SPAN = (int64_t)IV_SLICE * IV_SPAN_SLICES;
enum { IV_ENTRIES = 0, IV_POS = 1, IV_BASES = 15, IV_ALL = 29, IV_REF = 62, IV_CCS = 95, IV_OTHER = 32 };
static_assert(sizeof(himut_interval_row) == 1024 && sizeof(himut_interval_row) == IV_CELLS * sizeof(int64_t), "a row is 128 int64");
static_assert(offsetof(himut_interval_row, positions) == 8 * IV_POS && offsetof(himut_interval_row, bases) == 8 * IV_BASES &&
              offsetof(himut_interval_row, all_tri) == 8 * IV_ALL && offsetof(himut_interval_row, ref_tri) == 8 * IV_REF &&
              offsetof(himut_interval_row, ccs_tri) == 8 * IV_CCS, "the counters of a row in the order of its cells");
static_assert(IV_SLICE == HIMUT_CALLMAP_BLOCK, "the map's buffers carry a block of slack behind their last entry");
static_assert((uint64_t)IV_SPAN * 65535u < (1ull << 32), "a span's sum of bases fits a 32-bit cell");

// the callable run's geometry (the copies the intervals run keeps), its map, the reference string
struct IvGeo {
    const int32_t *cs, *ce;
    const int64_t* mapoff;
    int64_t nch;
    int ordered;                   // the chunks are ascending and disjoint
    const uint8_t* mstate;
    const uint16_t* mbases;
    const uint8_t* refseq;
    int64_t reflen;
};

// the entries [lo, hi) of chunk k inside (s, e); false: none
__device__ __forceinline__ bool iv_piece(const IvGeo& G, int64_t k, int32_t s, int32_t e, int64_t& lo, int64_t& hi) {
    const int32_t c = G.cs[k], a = max(s, c), b = min(e, G.ce[k]);
    if (a >= b) return false;
    lo = G.mapoff[k] + ((int64_t)a - c);
    hi = lo + ((int64_t)b - a);
    return true;
}

__device__ __forceinline__ int64_t iv_spans(int64_t lo, int64_t hi) { return hi > lo ? (hi - (lo & ~(int64_t)7) + IV_SPAN - 1) / IV_SPAN : 0; }

#ifndef HIMUT_INTERVALS_NO_KERNELS
__global__ void __launch_bounds__(256) k_iv_plan(IvGeo G, const int32_t* start, const int32_t* end, int64_t n, int64_t* lo, int64_t* hi,
                                                 int2* chunks, long long* cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) { cnt[n] = 0; return; }                       // (the scan runs over n + 1 counts: its last sum is the total)
    const int32_t s = start[i], e = end[i];
    int64_t a = 0, b = 0, c = 0;
    int2 ch = make_int2(0, 0);                                 // the chunks the interval's entries lie in: first, last
    if (s < e && G.ordered) {
        const int64_t first = upper_bound(G.ce, (int64_t)0, G.nch, s);   // the first chunk that ends behind s
        const int64_t last = lower_bound(G.cs, (int64_t)0, G.nch, e);    // the first chunk that starts at e or behind it
        if (first < last) {
            a = G.mapoff[first] + max((int64_t)s - G.cs[first], (int64_t)0);
            b = G.mapoff[last - 1] + ((int64_t)min(e, G.ce[last - 1]) - G.cs[last - 1]);
            c = iv_spans(a, b);
            ch = make_int2((int)first, (int)last - 1);
        }
    } else if (s < e) {
        for (int64_t k = 0; k < G.nch; k++) {
            int64_t plo, phi;
            if (iv_piece(G, k, s, e, plo, phi)) c += iv_spans(plo, phi);
        }
    }
    lo[i] = a; hi[i] = b; chunks[i] = ch; cnt[i] = (long long)c;
}
#endif  // HIMUT_INTERVALS_NO_KERNELS

__device__ __forceinline__ int iv_code(int c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }

// The class of the key normcounts.get_tri_context makes of three letters: a C or T centre as it stands, an A or G centre
// on the other strand; a letter outside upper-case ACGT anywhere: other.
__device__ __forceinline__ int iv_class(int t0, int t1, int t2) {
    const int a = iv_code(t0), m = iv_code(t1), b = iv_code(t2);
    if ((a | m | b) < 0) return IV_OTHER;
    if (m & 1) return a * 8 + (m == 3 ? 4 : 0) + b;
    return (3 - b) * 8 + (m == 0 ? 4 : 0) + (3 - a);
}

// byte k (a constant once unrolled) of the sixteen bytes (lo, hi)
__device__ __forceinline__ int iv_byte(uint64_t lo, uint64_t hi, int k) { return (int)(((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8)))) & 0xffu); }

// A thread's entries [i0, i0 + 8) of the map, i0 a multiple of 8 and below b: those inside [a, b) go to the cells.
// c0, c1: the chunks of entries a and b - 1.
__device__ __forceinline__ void iv_tally8(const IvGeo& G, uint32_t* cell, int64_t i0, int64_t a, int64_t b, int64_t c0, int64_t c1) {
    if (i0 + IV_PER <= a) return;
    // (both arrays carry a block of slack behind the map's last entry: aligned loads inside the buffers)
    const uint2 sv = *reinterpret_cast<const uint2*>(G.mstate + i0);
    const uint4 bv = *reinterpret_cast<const uint4*>(G.mbases + i0);
    const uint64_t s8 = (uint64_t)sv.x | ((uint64_t)sv.y << 32);
    const uint32_t bw[4] = {bv.x, bv.y, bv.z, bv.w};
    const int64_t mf = max(i0, a), ml = min(i0 + IV_PER, b);              // [mf, ml): this thread's entries of the span
    int64_t c = c0 == c1 ? c0 : upper_bound(G.mapoff, c0, c1 + 1, mf) - 1;   // the chunk of entry mf
    int64_t next = G.mapoff[c + 1];
    const int64_t rpos0 = (int64_t)G.cs[c] + (i0 - G.mapoff[c]);           // where entry i0 would lie in chunk c
    // the letters rpos0 - 1 .. rpos0 + 8 with four aligned loads, when the entries are of one chunk and far from the
    // string's ends; else a letter at a time
    const bool fast = ml <= next && rpos0 >= 1 && rpos0 + 15 <= G.reflen;
    uint64_t l0 = 0, l1 = 0;
    if (fast) {
        const int64_t p = rpos0 - 1;
        const int sh = 8 * (int)(p & 3);
        const uint32_t* w = reinterpret_cast<const uint32_t*>(G.refseq + (p & ~(int64_t)3));
        const uint64_t x = (uint64_t)w[0] | ((uint64_t)w[1] << 32), y = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
        l0 = sh ? (x >> sh) | (y << (64 - sh)) : x;
        l1 = y >> sh;
    }
    uint32_t run_s = 0xffu, run_n = 0, run_b = 0;                          // consecutive entries of one state: one update
#pragma unroll
    for (int k = 0; k < IV_PER; k++) {
        const int64_t m = i0 + k;
        if (m < mf || m >= ml) continue;
        int t0 = 'N', t1 = 'N', t2 = 'N';
        if (fast) {
            t0 = iv_byte(l0, l1, k); t1 = iv_byte(l0, l1, k + 1); t2 = iv_byte(l0, l1, k + 2);
        } else {
            while (m >= next) { c++; next = G.mapoff[c + 1]; }             // (chunks without a position are stepped over)
            const int64_t rpos = (int64_t)G.cs[c] + (m - G.mapoff[c]);
            if (rpos - 1 >= 0 && rpos + 2 <= G.reflen) { t0 = G.refseq[rpos - 1]; t1 = G.refseq[rpos]; t2 = G.refseq[rpos + 1]; }
        }
        const int cl = iv_class(t0, t1, t2);
        const uint32_t s = (uint32_t)(s8 >> (8 * k)) & 0xffu;
        const uint32_t nb = (bw[k >> 1] >> (16 * (k & 1))) & 0xffffu;
        atomicAdd(&cell[IV_ALL + cl], 1u);
        if (s == (uint32_t)HIMUT_CM_CALLABLE) {
            atomicAdd(&cell[IV_REF + cl], 1u);
            atomicAdd(&cell[IV_CCS + cl], nb);
        }
        if (s != run_s) {
            if (run_n && run_s < 14u) { atomicAdd(&cell[IV_POS + run_s], run_n); if (run_b) atomicAdd(&cell[IV_BASES + run_s], run_b); }
            run_s = s; run_n = 0; run_b = 0;
        }
        run_n++; run_b += nb;
    }
    if (run_n && run_s < 14u) { atomicAdd(&cell[IV_POS + run_s], run_n); if (run_b) atomicAdd(&cell[IV_BASES + run_s], run_b); }
}

#ifndef HIMUT_INTERVALS_NO_KERNELS
__global__ void __launch_bounds__(IV_NT) k_iv_tally(IvGeo G, const int32_t* start, const int32_t* end, int64_t n, const int64_t* lo,
                                                    const int64_t* hi, const int2* chunks, const long long* off, unsigned long long* rows) {
    __shared__ uint32_t cell[IV_CELLS];
    const int tid = threadIdx.x;
    const long long total = off[n];
    const long long per = (total + (long long)gridDim.x - 1) / (long long)gridDim.x;
    long long sp = (long long)blockIdx.x * per;
    const long long sp1 = min(sp + per, total);
    if (sp >= sp1) return;                                                 // (the same for every thread)
    int64_t i = upper_bound(off, (int64_t)0, n + 1, sp) - 1;               // the interval of span sp: off[i] <= sp < off[i + 1]
    for (; sp < sp1; sp++) {
        while (sp >= off[i + 1]) i++;                                      // (intervals without a span are stepped over)
        int64_t j = sp - off[i];                                           // the span's place among its interval's
        int64_t plo = 0, phi = 0, c0 = 0, c1 = 0;
        if (G.ordered) {
            plo = lo[i]; phi = hi[i];
        } else {                                                           // the slow path: the chunks again, up to the span's
            const int32_t s = start[i], e = end[i];
            for (int64_t k = 0; k < G.nch; k++) {
                if (!iv_piece(G, k, s, e, plo, phi)) continue;
                const int64_t here = iv_spans(plo, phi);
                c0 = c1 = k;
                if (j < here) break;
                j -= here;
            }
        }
        const int64_t base = (plo & ~(int64_t)7) + j * IV_SPAN;
        const int64_t a = max(plo, base), b = min(phi, base + IV_SPAN);
        if (G.ordered) {
            const int2 ch = chunks[i];
            c0 = c1 = ch.x;                                                // (an interval inside one chunk: no look-up)
            if (ch.x != ch.y) {
                c0 = upper_bound(G.mapoff, (int64_t)ch.x, (int64_t)ch.y + 1, a) - 1;
                c1 = upper_bound(G.mapoff, c0, (int64_t)ch.y + 1, b - 1) - 1;
            }
        }
        if (tid < IV_CELLS) cell[tid] = tid == IV_ENTRIES ? (uint32_t)(b - a) : 0u;
        __syncthreads();
        for (int64_t i0 = base + (int64_t)tid * IV_PER; i0 < b; i0 += IV_SLICE) iv_tally8(G, cell, i0, a, b, c0, c1);
        __syncthreads();
        if (tid < IV_CELLS) {
            const uint32_t v = cell[tid];
            if (v) atomicAdd(&rows[i * IV_CELLS + tid], (unsigned long long)v);
        }
        __syncthreads();
    }
}
#endif  // HIMUT_INTERVALS_NO_KERNELS

}  // namespace himut
