// Device code of the callable run (himut_run_callable): the normcounts verdict of every swept position kept per
// position -- a state byte and the position's callable bases -- and turned into runs of equal state on the device.
//
//   k_callmap_sweep    the map: k_norm_tile's sweep over every tile of every chunk (workgroup per 256-position tile, the
//                      reads' cells in LDS 48 rows at a time, a thread per column, the fp64 sums in fetch order), with the
//                      classification as the same text (NORM_CLASSIFY); every position writes its state and its bases
//   k_callmap_noreads  the map of a contig without reads: the reference letter decides (NON_ACGT or NO_BASE)
//   k_cm_reduce, k_cm_scan, k_cm_bounds, k_cm_records
//                      the runs: a boundary where a chunk starts or the state changes; the pair (boundaries, int64 sum
//                      of bases) scanned over the map -- per block of CM_BLOCK positions, over the blocks' totals, and
//                      again per block for the write; a run's bases is the difference of the scanned sums at its two
//                      ends.  The host reads the count between the scan and the write and sizes the records for it.
//
// The map holds the chunks one behind the other: entry mapoff[chunk] + (rpos - start[chunk]).
#pragma once

#define HIMUT_NORM_NO_KERNELS      // the arguments, the constants and the NORM_* text; the kernels are himut_norm.hip's
#include "himut_norm.h"

namespace himut {

static_assert(HIMUT_CALLMAP_TILE == 256, "the map sweep takes k_norm_tile's tiles");

// ---------------------------------------------------------------------------------------
// k_callmap_sweep: k_norm_tile without a list of tiles (grid: eight XCD classes x NT_Q workgroups, a row of the grid
// per chunk).  What differs from that kernel is behind the column walk: the verdict goes to the map.  The counters
// and the trinucleotide bins are kept as they fall out of the shared text (the run's log[14] is these counters).
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
    __shared__ double s_lut[3 * 257];         // three tables of 256 qualities + a zero entry each (index 256)
    __shared__ double s_prior[4];
    __shared__ unsigned int s_log[16];
    __shared__ unsigned int s_ccs[32], s_ref[32];
    __shared__ __align__(16) uint16_t s_cells[NT_ROWS][256];
    __shared__ int32_t s_tend[NT_ROWS];
    __shared__ uint32_t s_hap[NT_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wv = uni(tid >> 6);
    for (int i = tid; i < 3 * 256; i += 256) s_lut[(i >> 8) * 257 + (i & 255)] = A.lut->t[i >> 8][i & 255];
    if (tid < 3) s_lut[tid * 257 + 256] = 0.0;
    if (tid < 4) s_prior[tid] = A.lut->prior[tid];
    if (tid < 16) s_log[tid] = 0;
    if (tid < 32) { s_ccs[tid] = 0; s_ref[tid] = 0; }
    __syncthreads();
    const bool phase = A.P.p.phase != 0;
    const Reads& R = A.R;
    int bad = 0;
    // Which tile: workgroups are dealt round-robin over the eight XCDs (each with an L2 of its own), so the workgroups
    // b, b + 8, b + 16 ... that run side by side on one XCD take NEIGHBOURING tiles of the chunk: a read's bytes at a
    // tile boundary (its rows are 256 + 128 bytes at arbitrary offsets, i.e. partial 128-byte lines at both ends) are
    // then asked for twice within microseconds and the second time come out of that L2.  gridDim.x is a multiple of 8.
    // (Speed only: any mapping gives the same counts.)
    // A workgroup goes through several such tiles (its counters go to memory once): XCD class r = blockIdx.x & 7 owns the
    // tiles [r * per, (r + 1) * per) of the chunk and its NT_Q workgroups take NT_Q neighbouring ones per step.
    // (per: by THIS chunk's length -- with the longest chunk's figure a short chunk would sit on the first XCDs only)
    const int chunk = (int)blockIdx.y;
    const int64_t span = (int64_t)A.C.end[chunk] - (int64_t)A.C.start[chunk];
    const int64_t per = min(tiles_per_class, ((span + 255) / 256 + 7) / 8);
    const int64_t wg = (int64_t)(blockIdx.x >> 3), wgs = (int64_t)(gridDim.x >> 3);
    const int64_t mbase = mapoff[chunk];                         // the chunk's first entry of the map
    int too_deep = 0;
    for (int64_t t = wg; t < per; t += wgs) {
        const int32_t cs_ = A.C.start[chunk], ce_ = A.C.end[chunk];
        const int64_t pairbase = phase ? A.C.pairoff[chunk] - A.C.rlo[chunk] : 0;
        const int64_t tile = (int64_t)(blockIdx.x & 7) * per + t;
        const int64_t base = (int64_t)cs_ + tile * 256;
        if (base >= ce_) break;                                   // the same for every thread
        const int64_t rpos = base + tid;
        bool valid = rpos < ce_;
        if (valid && (rpos < 0 || rpos >= A.reflen)) { bad |= 1 << HIMUT_ERR_ARG; valid = false; }   // IndexError in the reference
        const int refc = valid ? (int)A.refseq[rpos] : 'N';
        const int ref = char2allele(refc);
        const bool edge = rpos <= cs_;
        const bool any_edge = base <= cs_;                       // only the chunk's first tile has such positions
        NORM_POS_STATE()
        uint32_t acc1 = 0, acc2 = 0;                              // 16-bit fields: insertions | deletions, reference | callable bases
        // rows: the reads of the window index of the blocks under the tile
        const int64_t b0 = min(max(base, (int64_t)0) >> WIN_SHIFT, nblk - 1), b1 = min((base + 255) >> WIN_SHIFT, nblk - 1);
        const int32_t lo = winlo[b0], hi = winhi[b1];
        const int32_t P0 = (int32_t)base + 4 * lane;              // this lane's four positions of every row
        for (int32_t r0 = lo; r0 < hi; r0 += NT_ROWS) {
            const int nb = min(NT_ROWS, hi - r0);
            // ---- the wave's rows, one per lane for the part that is a chain of dependent loads: read header, first
            //      segment that reaches the tile (binary search), the four segments from there on
            const int myrow = wv + 4 * lane;                      // rows wv, wv + 4, ... of the batch
            const bool rowlane = lane < NT_RPW && myrow < nb;
            ReadMeta M;
            M.tstart = 0; M.tend = 0; M.nseg = 0; M.flags = RF_SECONDARY; M.segbase = 0; M.qoff = 0;
            if (rowlane) M = D.meta[r0 + myrow];
            const bool live_row = rowlane && !(M.flags & RF_SECONDARY) && M.nseg > 0 && M.tstart < base + 256 && M.tend >= base;
            int j0 = 0;
            if (live_row) {                                       // last segment that starts at or before the tile
                int a = 0, e = M.nseg;
                while (a < e) { const int m = (a + e) >> 1; if (D.segs[M.segbase + m].t0 <= (int32_t)base) a = m + 1; else e = m; }
                j0 = max(a - 1, 0);
            }
            constexpr int NSG = HIMUT_NT_NSG;          // segments of a row kept in registers (the rest, rarely wanted, come from memory)
            int4 sg[NSG];
#pragma unroll
            for (int k = 0; k < NSG; k++) {
                sg[k] = make_int4(0x7fffffff, 0, 0, 0);
                if (live_row && j0 + k < M.nseg) sg[k] = *reinterpret_cast<const int4*>(D.segs + M.segbase + j0 + k);
            }
            if (rowlane) {
                s_tend[myrow] = M.tend;
                uint32_t hp = HAP_NONE;
                if (phase && live_row && M.tstart < ce_ && M.tend > cs_) hp = A.H.hap[pairbase + r0 + myrow];   // fetched by the chunk
                s_hap[myrow] = hp;
            }
            // ---- one row at a time, four positions per lane
            for (int l = 0; l < NT_RPW; l++) {
                const int row = wv + 4 * l;
                if (row >= nb) break;
                const bool rlive = lane_val((int)live_row, l) != 0;
                uint32_t cell[4] = {CELL_EMPTY, CELL_EMPTY, CELL_EMPTY, CELL_EMPTY};
                // nearly every row: one gapless segment spans the whole tile -- four bases straight from the three loads
                const int32_t f_t0 = lane_val(sg[0].x, l), f_len = lane_val(sg[0].z, l);
                const bool whole = rlive && !((uint32_t)lane_val(sg[0].w, l) & SEG_DEL) && f_t0 <= (int32_t)base &&
                                   (int64_t)f_t0 + f_len >= base + 256;
                if (whole) {
                    const int64_t qoff = ((int64_t)lane_val((int)(M.qoff >> 32), l) << 32) | (uint32_t)lane_val((int)M.qoff, l);
                    const int64_t K = qoff + lane_val(sg[0].y, l) + (P0 - f_t0);
                    uint32_t qv, sb;
                    __builtin_memcpy(&qv, R.bq + K, 4);
                    __builtin_memcpy(&sb, R.seq + (K >> 1), 4);
                    const uint64_t cw = (uint64_t)callable[K >> 5] | ((uint64_t)callable[(K >> 5) + 1] << 32);
                    const uint32_t cb = (uint32_t)(cw >> (K & 31));
                    // base K + y sits in byte (K + y) >> 1, high half when K + y is even: bring the four nibbles to bits 0..15
                    const uint32_t sw = __builtin_bswap32(sb);                 // bytes in nibble order
                    const uint32_t n4 = (K & 1) ? (sw >> 12) & 0xffffu : sw >> 16;   // base y at bits 12 - 4y .. 15 - 4y
#pragma unroll
                    for (int x = 0; x < 4; x++) {
                        const int nib = (int)((n4 >> (12 - 4 * x)) & 15u);
                        cell[x] = (uint32_t)nib2allele(nib) | (((qv >> (8 * x)) & 0xffu) << 8) | (((cb >> x) & 1u) << 4);
                    }
                    if (f_t0 == (int32_t)base && ((uint32_t)lane_val(sg[0].w, l) & SEG_INS) && lane == 0) cell[0] |= CELL_INS;
                } else if (rlive) {
                    const int ns = lane_val(M.nseg, l), jf = lane_val(j0, l);
                    const int64_t segbase = ((int64_t)lane_val((int)(M.segbase >> 32), l) << 32) | (uint32_t)lane_val((int)M.segbase, l);
                    const int64_t qoff = ((int64_t)lane_val((int)(M.qoff >> 32), l) << 32) | (uint32_t)lane_val((int)M.qoff, l);
                    for (int j = jf; j < ns; j++) {
                        int4 sv;
                        const int k = j - jf;
                        if (k < NSG) {
                            int4 c = sg[0];
#pragma unroll
                            for (int kk = 1; kk < NSG; kk++) if (k == kk) c = sg[kk];
                            sv = make_int4(lane_val(c.x, l), lane_val(c.y, l), lane_val(c.z, l), lane_val(c.w, l));
                        } else {
                            const Seg g = D.segs[segbase + j];
                            sv = make_int4(uni(g.t0), uni(g.q0), uni(g.len), uni((int)g.flags));
                        }
                        const int32_t t0 = sv.x, q0 = sv.y, len = sv.z;
                        const uint32_t fl = (uint32_t)sv.w;
                        if (t0 >= base + 256) break;
                        const int32_t span = len > 0 ? len : ((fl & SEG_INS) ? 1 : 0);      // a trailing insertion marks one position
                        const int32_t a = max(P0, t0), e = min(P0 + 4, t0 + span);
                        if (a >= e) continue;
                        if (fl & SEG_DEL) {
#pragma unroll
                            for (int x = 0; x < 4; x++)
                                if (P0 + x >= a && P0 + x < e) cell[x] = CELL_DEL | ((P0 + x == t0 && (fl & SEG_INS)) ? CELL_INS : 0u);
                        } else if (len == 0) {
#pragma unroll
                            for (int x = 0; x < 4; x++) if (P0 + x == t0) cell[x] = CELL_EMPTY | CELL_INS;
                        } else {
                            // up to four consecutive query bases from K on: qualities, packed bases (high nibble first) and
                            // callable bits, each with one unaligned load (the buffers carry slack behind the last read)
                            const int64_t K = qoff + q0 + (a - t0);
                            uint32_t qv, sb;
                            __builtin_memcpy(&qv, R.bq + K, 4);
                            __builtin_memcpy(&sb, R.seq + (K >> 1), 4);
                            const uint64_t cw = (uint64_t)callable[K >> 5] | ((uint64_t)callable[(K >> 5) + 1] << 32);
                            const uint32_t cb = (uint32_t)(cw >> (K & 31));
                            // nibble of base K + y: byte (K + y) >> 1, high half when K + y is even
                            const uint32_t odd = (uint32_t)(K & 1);
#pragma unroll
                            for (int x = 0; x < 4; x++) {
                                const int y = P0 + x - a;                                   // index among the loaded bases
                                if (y >= 0 && P0 + x < e) {
                                    const uint32_t kk = (uint32_t)y + odd;                  // nibble index from the first loaded byte
                                    const uint32_t byte = (sb >> (8 * (kk >> 1))) & 0xffu;
                                    const int nib = (kk & 1) ? (int)(byte & 15u) : (int)(byte >> 4);
                                    uint32_t val = (uint32_t)nib2allele(nib) | (((qv >> (8 * y)) & 0xffu) << 8) | (((cb >> y) & 1u) << 4);
                                    if (P0 + x == t0 && (fl & SEG_INS)) val |= CELL_INS;
                                    cell[x] = val;
                                }
                            }
                        }
                    }
                }
                uint2 packed;
                packed.x = cell[0] | (cell[1] << 16);
                packed.y = cell[2] | (cell[3] << 16);
                *reinterpret_cast<uint2*>(&s_cells[row][4 * lane]) = packed;
            }
            __syncthreads();
            // ---- every thread down its column, in read order
            if (valid) {
                // NB rows at a time: the cells, then the three table values of each (the zero row unless the cell is the
                // reference allele), are loaded before any of them is used: the LDS latency is paid once per NB cells
                constexpr int NB = 2;      // (four at a time costs more in spills than the extra LDS round trips save)
                for (int i0 = 0; i0 < nb; i0 += NB) {
                    uint32_t v4[NB];
                    double th[NB], tt[NB], te[NB];
                    bool use4[NB], ref4[NB];
#pragma unroll
                    for (int k = 0; k < NB; k++) v4[k] = i0 + k < nb ? (uint32_t)s_cells[i0 + k][tid] : (uint32_t)CELL_EMPTY;
#pragma unroll
                    for (int k = 0; k < NB; k++) {
                        const uint32_t v = v4[k];
                        const int ri = min(i0 + k, nb - 1);
                        // an EMPTY cell, or a read this chunk did not fetch (normcounts.py:289), adds nothing
                        use4[k] = (v & 15u) != CELL_EMPTY && !(any_edge && edge && !(s_tend[ri] > cs_));
                        ref4[k] = use4[k] && (int)(v & 7u) == ref;
                        const uint32_t qe = ref4[k] ? (v >> 8) : 256u;      // the zero row for everything but the reference allele
                        th[k] = s_lut[qe]; tt[k] = s_lut[257 + qe]; te[k] = s_lut[514 + qe];
                    }
#pragma unroll
                    for (int k = 0; k < NB; k++)
                        NORM_CELL_Z(v4[k], use4[k], ref4[k], s_hap[min(i0 + k, nb - 1)], th[k], tt[k], te[k], acc1, acc2)
                }
            }
            __syncthreads();
            if (((r0 - lo) / NT_ROWS & 511) == 511) {             // a pile tens of thousands of reads deep: empty the 16-bit fields
                cnt[4] += acc1 & 0xffffu; cnt[5] += acc1 >> 16; nref += acc2 & 0xffffu; tri_sum += acc2 >> 16;
                acc1 = 0; acc2 = 0;
            }
        }
        if (rpos >= ce_) continue;
        cnt[4] += acc1 & 0xffffu; cnt[5] += acc1 >> 16; nref += acc2 & 0xffffu; tri_sum += acc2 >> 16;
        // The verdict.  NORM_CLASSIFY leaves through `continue` where the reference's loop does (no reference base, no
        // base, unphased; a zero quality, which fails the run): inside a loop of one round that ends the round, and the
        // state set in front of it stands.  A position that comes out of its end is in row `slot` of norm.log.
        uint32_t st = (ref < 0 || !valid) ? (uint32_t)HIMUT_CM_NON_ACGT : tri_sum == 0 ? (uint32_t)HIMUT_CM_NO_BASE : (uint32_t)HIMUT_CM_UNPHASED;
        for (int once = 0; once < 1; once++) {
            NORM_CLASSIFY()
            st = (uint32_t)slot;
        }
        const uint32_t nb16 = st <= (uint32_t)HIMUT_CM_NO_BASE ? 0u : tri_sum;
        if (nb16 > 0xffffu) too_deep = 1;                         // (the host fails the run: nothing is stored cut short)
        const int64_t m = mbase + (rpos - cs_);
        mstate[m] = (uint8_t)st;                                  // a wave's 64 bytes / 128 bytes, one behind the other
        mbases[m] = (uint16_t)min(nb16, 0xffffu);
    }
    if (too_deep) *deep = 1;
    __syncthreads();
    if (tid < 14 && s_log[tid]) atomicAdd(&A.log[tid], (unsigned long long)s_log[tid]);
    if (tid < 32 && (s_ccs[tid] || s_ref[tid])) {
        const int cl[4] = {A.cA, A.cC, A.cG, A.cT};
        const int64_t k = ((int64_t)cl[tid >> 3] * A.K + ((tid & 4) ? A.cT : A.cC)) * A.K + cl[tid & 3];
        atomicAdd(&A.ccs_tri[k], (unsigned long long)s_ccs[tid]);
        atomicAdd(&A.ref_tri[k], (unsigned long long)s_ref[tid]);
    }
    if (bad) atomicOr(A.err, bad);
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
