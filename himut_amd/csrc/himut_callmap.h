// Device code of the callable run (himut_run_callable): the normcounts verdict of every swept position kept per
// position -- a state byte and the position's callable bases -- and turned into runs of equal state on the device.
//
//   k_callmap_sweep    the map: the tile sweep of himut_sweep.h, which k_norm_tile runs too, over every tile of every
//                      chunk (workgroup per 256-position tile, the reads' cells in LDS 48 rows at a time, a thread per
//                      column, the fp64 sums in fetch order) and its classification (norm_classify); every position
//                      writes its state and its bases
//   k_callmap_noreads  the map of a contig without reads: the reference letter decides (NON_ACGT or NO_BASE)
//   k_cm_reduce, k_cm_scan, k_cm_bounds, k_cm_records
//                      the runs: a boundary where a chunk starts or the state changes; the pair (boundaries, int64 sum
//                      of bases) scanned over the map -- per block of CM_BLOCK positions, over the blocks' totals, and
//                      again per block for the write; a run's bases is the difference of the scanned sums at its two
//                      ends.  The host reads the count between the scan and the write and sizes the records for it.
//
// The map holds the chunks one behind the other: entry mapoff[chunk] + (rpos - start[chunk]).
#pragma once

#include "himut_sweep.h"

namespace himut {

static_assert(HIMUT_CALLMAP_TILE == 256, "the map sweep takes k_norm_tile's tiles");
static_assert(HIMUT_CM_NON_ACGT == NORM_V_NO_REF && HIMUT_CM_NO_BASE == NORM_V_NO_BASE && HIMUT_CM_UNPHASED == NORM_V_UNPHASED &&
              HIMUT_CM_HET == 3 && HIMUT_CM_INDEL == 7 && HIMUT_CM_CALLABLE == 13, "a state of the map is the verdict norm_classify returns");

// ---------------------------------------------------------------------------------------
// k_callmap_sweep: the tile sweep over every tile of every chunk (grid: eight XCD classes x NT_Q workgroups, a row of
// the grid per chunk), as k_norm_tile runs it without a list.  What differs from that kernel is behind the verdict: it
// goes to the map.  The counters and the trinucleotide bins are kept as norm_classify and norm_tally leave them (the
// run's log[14] is these counters).
// A pile deeper than a 16-bit count: the walk empties its 16-bit fields into 32-bit counters every 512 batches, as the
// normcounts run does, so the verdict and the counters are exact at any depth; only the map's field is 16 bits, and a
// position that does not fit it sets *deep.
// Four waves per SIMD, one fewer than k_norm_tile asks for: with that kernel's 96 registers the verdict's extra state
// spills (48 bytes of scratch a lane); with 128 nothing does.
#ifndef HIMUT_CM_SWEEP_WAVES
#define HIMUT_CM_SWEEP_WAVES 4
#endif
constexpr int CM_SWEEP_WAVES = HIMUT_CM_SWEEP_WAVES;
__global__ void __launch_bounds__(256, CM_SWEEP_WAVES) k_callmap_sweep(NormArgs A, Derived D, const uint32_t* callable, const int32_t* winlo,
                                                   const int32_t* winhi, int64_t nblk, int64_t tiles_per_class, const int64_t* mapoff,
                                                   uint8_t* mstate, uint16_t* mbases, int* deep) {
    __shared__ NormLds L;
    norm_lds_init(L, A);
    const bool phase = A.P.p.phase != 0;
    int bad = 0;
    const int chunk = (int)blockIdx.y;
    const int64_t per = norm_tiles_per_class(A, chunk, tiles_per_class);
    const int64_t mbase = mapoff[chunk];                         // the chunk's first entry of the map
    int too_deep = 0;
    for (int64_t t = (int64_t)(blockIdx.x >> 3); t < per; t += (int64_t)(gridDim.x >> 3)) {
        const int32_t cs_ = A.C.start[chunk], ce_ = A.C.end[chunk];
        const int64_t base = (int64_t)cs_ + ((int64_t)(blockIdx.x & 7) * per + t) * 256;
        if (base >= ce_) break;                                   // the same for every thread
        const NormTile T = norm_tile_at(A, chunk, base, cs_, ce_, winlo, winhi, nblk, phase, bad);
        NormPos p;
        norm_sweep_tile(L, A, D, callable, T, p, phase, bad);
        if (T.rpos >= ce_) continue;
        // (a position outside the reference string has no reference base: NON_ACGT; a zero quality fails the run, and
        //  its position's entry, which nobody gets to see, is UNPHASED)
        const int verdict = norm_classify(p, A, L.tally, T.ref, T.rpos, phase, bad);
        norm_tally(verdict, p.tri_sum, A, L.tally, T.rpos, T.refc);
        const uint32_t st = verdict == NORM_V_BQ0 ? (uint32_t)HIMUT_CM_UNPHASED : (uint32_t)verdict;
        const uint32_t nb16 = st <= (uint32_t)HIMUT_CM_NO_BASE ? 0u : p.tri_sum;
        if (nb16 > 0xffffu) too_deep = 1;                         // (the host fails the run: nothing is stored cut short)
        const int64_t m = mbase + (T.rpos - cs_);
        mstate[m] = (uint8_t)st;                                  // a wave's 64 bytes / 128 bytes, one behind the other
        mbases[m] = (uint16_t)min(nb16, 0xffffu);
    }
    if (too_deep) *deep = 1;
    norm_flush(L.tally, A, bad);
}

// ---------------------------------------------------------------------------------------
// The runs.  A workgroup of CM_NT threads takes CM_BLOCK consecutive entries of the map, a thread CM_PER consecutive ones.
constexpr int CM_BLOCK = HIMUT_CALLMAP_BLOCK, CM_NT = 256, CM_PER = CM_BLOCK / CM_NT;
static_assert(CM_PER == 8, "a thread loads its eight states and bases with one vector load each");

struct CmPair { long long cnt, sum; };            // boundaries, bases: of a block, then (scanned) in front of the block
struct CmScalars { long long nruns, total; int deep; int pad[3]; };

__global__ void __launch_bounds__(256) k_callmap_noreads(const uint8_t* refseq, int64_t reflen, const int32_t* cstart, const int64_t* mapoff,
                                                         int64_t nchunks, int64_t N, uint8_t* mstate, uint16_t* mbases, int* err) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int64_t c = upper_bound(mapoff, (int64_t)0, nchunks + 1, i) - 1;
    const int64_t rpos = (int64_t)cstart[c] + (i - mapoff[c]);
    int ref = -1;
    if (rpos < 0 || rpos >= reflen) set_err(err, HIMUT_ERR_ARG);          // IndexError in the reference
    else ref = char2allele((int)refseq[rpos]);
    mstate[i] = (uint8_t)(ref < 0 ? HIMUT_CM_NON_ACGT : HIMUT_CM_NO_BASE);
    mbases[i] = 0;
}

// A thread's entries [i0, i0 + 8) of the map: bit k of the result is set where entry i0 + k starts a run (the map's
// first entry, a chunk's first entry, a state other than the entry's in front); b[k]: its bases (0 behind the map's end).
// s_c[0], s_c[1]: the chunks of the block's first and last entry (found once per block, cm_block_chunks).
__device__ __forceinline__ uint32_t cm_items(const uint8_t* mstate, const uint16_t* mbases, const int64_t* mapoff, const int64_t* s_c,
                                             int64_t N, int64_t i0, uint32_t (&b)[CM_PER]) {
#pragma unroll
    for (int k = 0; k < CM_PER; k++) b[k] = 0;
    if (i0 >= N) return 0u;
    // (both arrays carry CM_BLOCK entries of slack behind N and i0 is a multiple of 8: aligned loads inside the buffers)
    const uint2 sv = *reinterpret_cast<const uint2*>(mstate + i0);
    const uint4 bv = *reinterpret_cast<const uint4*>(mbases + i0);
    const uint32_t bw[4] = {bv.x, bv.y, bv.z, bv.w};
    const uint64_t s8 = (uint64_t)sv.x | ((uint64_t)sv.y << 32);
    uint32_t prev = i0 > 0 ? (uint32_t)mstate[i0 - 1] : 0xffu;
    int64_t c = upper_bound(mapoff, s_c[0], s_c[1] + 1, i0) - 1;          // the chunk of entry i0
    int64_t next = mapoff[c + 1];
    uint32_t flags = 0;
#pragma unroll
    for (int k = 0; k < CM_PER; k++) {
        const int64_t i = i0 + k;
        if (i >= N) break;
        while (i >= next) { c++; next = mapoff[c + 1]; }                   // (chunks without a position are stepped over)
        const uint32_t s = (uint32_t)(s8 >> (8 * k)) & 0xffu;
        if (i == mapoff[c] || s != prev) flags |= 1u << k;
        prev = s;
        b[k] = (bw[k >> 1] >> (16 * (k & 1))) & 0xffffu;
    }
    return flags;
}

__device__ __forceinline__ void cm_block_chunks(const int64_t* mapoff, int64_t nchunks, int64_t N, int64_t* s_c) {
    if (threadIdx.x == 0) {
        const int64_t first = (int64_t)blockIdx.x * CM_BLOCK, last = min(first + CM_BLOCK, N) - 1;
        s_c[0] = upper_bound(mapoff, (int64_t)0, nchunks + 1, first) - 1;
        s_c[1] = upper_bound(mapoff, (int64_t)0, nchunks + 1, last) - 1;
    }
    __syncthreads();
}

// the workgroup's inclusive scan of (v0, v1), both sums below 2^31 within a block (2048 x 65,535 bases)
__device__ __forceinline__ void cm_block_scan(uint32_t& v0, uint32_t& v1, uint32_t* s_w) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    v0 = (uint32_t)wave_incl_add((int)v0, lane);
    v1 = (uint32_t)wave_incl_add((int)v1, lane);
    if (lane == 63) { s_w[wv] = v0; s_w[4 + wv] = v1; }
    __syncthreads();
    for (int w = 0; w < wv; w++) { v0 += s_w[w]; v1 += s_w[4 + w]; }
}

__global__ void __launch_bounds__(CM_NT) k_cm_reduce(const uint8_t* mstate, const uint16_t* mbases, const int64_t* mapoff, int64_t nchunks,
                                                     int64_t N, CmPair* blk) {
    __shared__ int64_t s_c[2];
    __shared__ uint32_t s_w[8];
    cm_block_chunks(mapoff, nchunks, N, s_c);
    uint32_t b[CM_PER];
    const uint32_t flags = cm_items(mstate, mbases, mapoff, s_c, N, (int64_t)blockIdx.x * CM_BLOCK + (int64_t)threadIdx.x * CM_PER, b);
    uint32_t v0 = (uint32_t)__builtin_popcount(flags), v1 = 0;
#pragma unroll
    for (int k = 0; k < CM_PER; k++) v1 += b[k];
    cm_block_scan(v0, v1, s_w);
    if (threadIdx.x == CM_NT - 1) { CmPair p; p.cnt = (long long)v0; p.sum = (long long)v1; blk[blockIdx.x] = p; }
}

// one workgroup: the blocks' totals become what lies in front of each block; the totals of the map go to sc
constexpr int CM_SCAN_NT = 1024;
__global__ void __launch_bounds__(CM_SCAN_NT) k_cm_scan(CmPair* blk, int64_t nblocks, CmScalars* sc) {
    __shared__ long long s_cnt[CM_SCAN_NT], s_sum[CM_SCAN_NT];
    const int tid = threadIdx.x;
    const int64_t per = (nblocks + CM_SCAN_NT - 1) / CM_SCAN_NT;
    const int64_t lo = min((int64_t)tid * per, nblocks), hi = min(lo + per, nblocks);
    long long cnt = 0, sum = 0;
    for (int64_t k = lo; k < hi; k++) { const CmPair p = blk[k]; cnt += p.cnt; sum += p.sum; }
    s_cnt[tid] = cnt; s_sum[tid] = sum;
    __syncthreads();
    for (int d = 1; d < CM_SCAN_NT; d <<= 1) {
        const long long a = tid >= d ? s_cnt[tid - d] : 0, b = tid >= d ? s_sum[tid - d] : 0;
        __syncthreads();
        s_cnt[tid] += a; s_sum[tid] += b;
        __syncthreads();
    }
    long long c0 = s_cnt[tid] - cnt, u0 = s_sum[tid] - sum;                 // in front of this thread's blocks
    for (int64_t k = lo; k < hi; k++) {
        const CmPair p = blk[k];
        CmPair q; q.cnt = c0; q.sum = u0;
        blk[k] = q;
        c0 += p.cnt; u0 += p.sum;
    }
    if (tid == CM_SCAN_NT - 1) { sc->nruns = s_cnt[tid]; sc->total = s_sum[tid]; }
}

// run r starts at entry bnd[r].cnt of the map with bnd[r].sum bases in front of it; bnd[nruns] closes the last run
__global__ void __launch_bounds__(CM_NT) k_cm_bounds(const uint8_t* mstate, const uint16_t* mbases, const int64_t* mapoff, int64_t nchunks,
                                                     int64_t N, const CmPair* blk, const CmScalars* sc, CmPair* bnd) {
    __shared__ int64_t s_c[2];
    __shared__ uint32_t s_w[8];
    cm_block_chunks(mapoff, nchunks, N, s_c);
    uint32_t b[CM_PER];
    const int64_t i0 = (int64_t)blockIdx.x * CM_BLOCK + (int64_t)threadIdx.x * CM_PER;
    const uint32_t flags = cm_items(mstate, mbases, mapoff, s_c, N, i0, b);
    const uint32_t n0 = (uint32_t)__builtin_popcount(flags);
    uint32_t n1 = 0;
#pragma unroll
    for (int k = 0; k < CM_PER; k++) n1 += b[k];
    uint32_t v0 = n0, v1 = n1;
    cm_block_scan(v0, v1, s_w);
    const CmPair front = blk[blockIdx.x];
    long long r = front.cnt + (long long)(v0 - n0), u = front.sum + (long long)(v1 - n1);
    const long long nruns = sc->nruns;
#pragma unroll
    for (int k = 0; k < CM_PER; k++) {
        if ((flags >> k) & 1u) {
            if (r < nruns) { CmPair p; p.cnt = i0 + k; p.sum = u; bnd[r] = p; }     // (r < nruns always: the same flags were counted)
            r++;
        }
        u += b[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { CmPair p; p.cnt = N; p.sum = sc->total; bnd[nruns] = p; }
}

__global__ void __launch_bounds__(256) k_cm_records(const uint8_t* mstate, const int64_t* mapoff, const int32_t* cstart, int64_t nchunks,
                                                    const CmPair* bnd, int64_t nruns, himut_callable_run* runs) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nruns) return;
    const CmPair a = bnd[r], e = bnd[r + 1];
    const int64_t c = upper_bound(mapoff, (int64_t)0, nchunks + 1, (int64_t)a.cnt) - 1;
    himut_callable_run o;
    o.chunk = (int32_t)c;
    o.start = (int32_t)((int64_t)cstart[c] + (a.cnt - mapoff[c]));
    o.end = (int32_t)((int64_t)o.start + (e.cnt - a.cnt));
    o.state = (int32_t)mstate[a.cnt];
    o.bases = e.sum - a.sum;
    runs[r] = o;
}

}  // namespace himut
