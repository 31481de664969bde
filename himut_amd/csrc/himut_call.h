// Device code of the call run: what it launches behind the column front (himut_front.h), whose capture has left the
// column store and, from the reads' proposals, a mask of (chunk, tpos, ref, alt) bits (by chunk cell: with their count per tile).
// do_run_once (himut_call.hip) launches them in order; DESIGN.md sections 2-4.
//
//   k_mask_count / k_mask_emit
//                      chunks in coordinate order (the reference's own, phase blocks): the set bits of the mask by column
//                      rank, a thread per 256-position block, counted per tile and then written out in (tpos, chunk,
//                      ref, alt) order = the candidate list in the order of the final records
//   k_scan_small / k_mask_emit_cells
//                      any other chunk list: the set bits of the mask by chunk cell in (chunk, tpos, ref, alt) order,
//                      radix-sorted afterwards
//   k_eval_columns     one THREAD per candidate column: the shared column walk, genotype and non-phased cascade
//                      (himut_column.h) under the chunk's fetch rule, then the haplotype vote (--phase)
//                      (caller.py:44-72,324-621, bamlib.py:181-219, gtlib.py:72-174)
//   k_finalize_flags / k_run_totals / k_compact
//                      cross-chunk som_seen (caller.py:244,347, bamlib.py:77), the 15 counters (caller.py:625-641),
//                      set() de-duplication (caller.py:622-624), the totals, the emitted records to the front
// (the record's packing, a thread's place among its workgroup's records, the front's totals: himut_emit.h, as in germline and dbs)
//
// Integer work plus a small fp64 tail; no MFMA.  Wave size 64 throughout.
#pragma once

#include "himut_emit.h"

namespace himut {

// ---------------------------------------------------------------------------------------
// The candidate list = the set bits of the mask (16 bits per cell: one per (ref, alt)).  Cells
// with a bit are few (one in ~150 at 30x) and all of them sit at column positions, so the two
// sweeps read the position bitmap (k_parse_cs) instead of the mask and look only at the cells of
// marked positions: bits per tile of 8192 cells (32 cells per thread), then -- after a scan of
// the tile counts -- the candidates themselves, in mask order: chunk, position, then (ref, alt)
// in ASCII order.  The sort key of a candidate == the sort key of its record: (tpos, chunk, ref,
// alt), natsorted order of the reference's tuples (caller.py:622).  The emit sweep leaves the
// mask zeroed for the next run.

// where a thread of the sweeps stands in the chunk list
struct CellCursor {
    int64_t ck, cbeg, cend;   // chunk of the cell, its first cell, first cell of the next chunk
    int32_t cstart;           // the chunk's start (tpos of cell cbeg)
};

// Summary word of the mask cells [32 i, 32 i + 32): bit b set when the cell's position (rpos = tpos - 1) is a
// column position.  cur: the chunk of the tile's first cell on entry, of cell 32 i on return.
__device__ __forceinline__ uint32_t cell_summary(const Chunks& C, const uint32_t* posbits, int64_t i, int64_t ncells, CellCursor& cur) {
    const int64_t c0 = i * 32;
    if (c0 >= ncells) return 0u;
    while (c0 >= cur.cend) { cur.ck++; cur.cbeg = cur.cend; cur.cend = C.maskoff[cur.ck + 1]; cur.cstart = C.start[cur.ck]; }
    if (c0 + 32 <= cur.cend) {                       // the 32 cells lie in one chunk: 32 consecutive positions
        const int64_t rp = (int64_t)cur.cstart + (c0 - cur.cbeg) - 1;
        if (rp < 0) return posbits[0] << 1;          // cell of tpos 0 (a chunk that starts at 0): no such position
        const uint32_t lo = posbits[rp >> 5], hi = posbits[(rp >> 5) + 1];
        const int sh = (int)(rp & 31);
        return sh ? ((lo >> sh) | (hi << (32 - sh))) : lo;
    }
    uint32_t w = 0;
    CellCursor t = cur;
    for (int b = 0; b < 32 && c0 + b < ncells; b++) {
        const int64_t c = c0 + b;
        while (c >= t.cend) { t.ck++; t.cbeg = t.cend; t.cend = C.maskoff[t.ck + 1]; t.cstart = C.start[t.ck]; }
        const int64_t rp = (int64_t)t.cstart + (c - t.cbeg) - 1;
        if (rp >= 0 && ((posbits[rp >> 5] >> (rp & 31)) & 1u)) w |= 1u << b;
    }
    return w;
}

// the candidates of one mask cell (m: its bits, none past bit 15) from `slot` on, which moves behind them
__device__ __forceinline__ void emit_cell(uint32_t m, int32_t tpos, int64_t ck, Cand* cands, uint64_t* keys, int64_t cap, int64_t& slot) {
    // (ref, alt) in ASCII order A C G T = alleles 0 3 2 1: bit rk of x is bit (ref << 2 | alt) of m -- bits 1 and 3 of
    // every nibble change places, then nibbles 1 and 3.  A cell nearly always holds one bit: a turn per bit, not sixteen
    uint32_t x = (m & 0x5555u) | ((m & 0x2222u) << 2) | ((m & 0x8888u) >> 2);
    x = (x & 0x0f0fu) | ((x & 0x00f0u) << 8) | ((x & 0xf000u) >> 8);
    for (; x; x &= x - 1) {
        const int rk = __ffs((int)x) - 1;
        const int ra = (0x1230 >> (4 * (rk >> 2))) & 15, aa = (0x1230 >> (4 * (rk & 3))) & 15;
        const int bit = (ra << 2) | aa;
        if (slot < cap) {
            Cand cd; cd.tpos = tpos; cd.chunk_bit = ((uint32_t)ck << 4) | (uint32_t)bit;
            cands[slot] = cd;
            keys[slot] = ((uint64_t)(uint32_t)tpos << 28) | ((uint64_t)ck << 4) | (uint64_t)rk;
        }
        slot++;
    }
}

// cap: capacity of cands / keys (the host may have sized them before the count was known: nothing is
// written past it, and the true count lands in *total for the host to compare with cap)
// tilecnt: the tile counts the proposals made (propose_read; their scan is tileoff); zeroed here for the next run, like the mask.
__global__ void __launch_bounds__(256) k_mask_emit_cells(const uint32_t* posbits, int64_t ncells, uint16_t* mask16, const uint32_t* tileoff,
                                                         Chunks C, Cand* cands, uint64_t* keys, int64_t cap, unsigned long long* total,
                                                         uint32_t* tilecnt) {
    __shared__ int s_w[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x == 0) tilecnt[blockIdx.x] = 0;
    // the chunk of the tile's first cell comes with the tile; cells may run into the next chunks
    const MaskTile mt = C.mtile[blockIdx.x];
    CellCursor cur = {mt.ck0, mt.off0, mt.off1, mt.start0};
    uint32_t w = cell_summary(C, posbits, i, ncells, cur);
    int c = 0;
    for (uint32_t x = w; x; x &= x - 1) c += __popc((uint32_t)mask16[i * 32 + (__ffs((int)x) - 1)]);
    const int incl = wave_incl_add(c, lane);
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
        *total = (unsigned long long)tileoff[blockIdx.x] + (unsigned long long)(s_w[0] + s_w[1] + s_w[2] + s_w[3]);
    if (!c) return;
    int64_t slot = (int64_t)tileoff[blockIdx.x] + (incl - c);
#pragma unroll
    for (int k = 0; k < 4; k++) if (k < wv) slot += s_w[k];
    int64_t ck = cur.ck;
    int64_t cbeg = cur.cbeg, cend_ = cur.cend;
    int32_t cstart = cur.cstart;
    while (w) {
        const int b = __ffs((int)w) - 1; w &= w - 1;
        const int64_t cell = i * 32 + b;
        const uint32_t m = mask16[cell];
        if (!m) continue;
        mask16[cell] = 0;
        while (cell >= cend_) { ck++; cbeg = cend_; cend_ = C.maskoff[ck + 1]; cstart = C.start[ck]; }
        emit_cell(m, cstart + (int32_t)(cell - cbeg), ck, cands, keys, cap, slot);
    }
}

// The same list from a mask indexed by column rank (chunks in order): the cell of (chunk k, position p) is
// rmask[u(p) + k], u the position's number among the marked positions, so the cells of a 256-position block's marked
// positions are neighbours and the whole mask is a few hundred kB.  The grids are k_block_table3's: a thread takes `per`
// consecutive blocks, a workgroup's blocks are one tile.  k_mask_count leaves the set bits of every tile, k_mask_emit
// adds up the tiles in front of its own, as k_block_table3 does with its totals, and writes the candidates out.  (The
// proposals do not count the bits they set: 4 * 10^5 atomic adds on the few counters under the reads in flight doubled
// the capture's time, profiles/README.md "Rank mask".)
struct RankMask {
    PosIndex X;
    uint16_t* cells;           // rmask
    int64_t ncells;            // cells the mask holds (none is touched past them)
    const int32_t *cstart, *cend;
    int64_t nch;               // chunks, in order
    const int32_t* blkchunk;   // per block the first chunk that ends at or behind the block's first tpos (upload_chunks)
    int64_t nbc;               // ... for this many blocks; behind them no chunk
};

// One block's share of the mask: its bitmap words, where its cells begin, its place in the chunk list.
struct RankBlock {
    uint32_t w[8];                    // the block's bitmap words (all zero: nothing to do)
    uint32_t u0;                      // rank of its first marked position
    int64_t k;                        // chunk k, [ks, ke], and the start of the next one
    int32_t ks, ke, kn, t0;           // t0: tpos of the block's first position
    bool one;                         // the block lies inside chunk k and no other (nearly every one)
    unsigned long long pre[2];        // one: its first eight cells, loaded together

    // the loads do not depend on each other: bitmap, chunk and rank first, then the chunk's edges, then the cells
    __device__ __forceinline__ void load(const RankMask& M, int64_t b) {
        const uint4* wp = reinterpret_cast<const uint4*>(M.X.bits + (b << 3));
        const uint4 x = wp[0], y = wp[1];
        k = b < M.nbc ? (int64_t)M.blkchunk[b] : M.nch;
        u0 = M.X.bt[b].ufirst;
        t0 = (int32_t)(b << 8) + 1;
        const bool any = (x.x | x.y | x.z | x.w | y.x | y.y | y.z | y.w) != 0u && k < M.nch;    // (behind the last chunk: no cells)
        w[0] = any ? x.x : 0u; w[1] = any ? x.y : 0u; w[2] = any ? x.z : 0u; w[3] = any ? x.w : 0u;
        w[4] = any ? y.x : 0u; w[5] = any ? y.y : 0u; w[6] = any ? y.z : 0u; w[7] = any ? y.w : 0u;
        one = false; pre[0] = pre[1] = 0ull; ks = ke = kn = 0x7fffffff;
        if (!any) return;
        ks = M.cstart[k]; ke = M.cend[k]; kn = k + 1 < M.nch ? M.cstart[k + 1] : 0x7fffffff;
        one = ks <= t0 && t0 + 255 <= ke && kn > t0 + 255;
        if (one) {
            const int64_t c0 = (int64_t)u0 + k;
            const int cnt = __popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]) + __popc(w[4]) + __popc(w[5]) + __popc(w[6]) + __popc(w[7]);
            uint32_t m8[8];
#pragma unroll
            for (int j = 0; j < 8; j++) m8[j] = (j < cnt && c0 + j < M.ncells) ? (uint32_t)M.cells[c0 + j] : 0u;
#pragma unroll
            for (int j = 0; j < 8; j++) pre[j >> 2] |= (unsigned long long)m8[j] << (16 * (j & 3));
        }
    }

    // The block's cells in (tpos, chunk) order.  EMIT: writes the candidates of the set ones from `slot` on and zeroes
    // them; else only counts their bits.  Returns the bits.
    template <bool EMIT>
    __device__ __forceinline__ int walk(const RankMask& M, Cand* cands, uint64_t* keys, int64_t cap, int64_t& slot) const {
        int bits = 0;
        uint32_t j = 0;                                           // marked positions of the block in front of this one
        int64_t kc = k;
        int32_t cs_ = ks, ce_ = ke, cn_ = kn;
        auto cell_of = [&](const int64_t cell, const int32_t tpos, const int64_t ck, const bool first8) {
            uint32_t m;
            if (first8) m = (uint32_t)((j < 4 ? pre[0] : pre[1]) >> (16 * (j & 3))) & 0xffffu;
            else m = cell < M.ncells ? (uint32_t)M.cells[cell] : 0u;
            if (!m) return;
            if (EMIT) { M.cells[cell] = 0; emit_cell(m, tpos, ck, cands, keys, cap, slot); }
            else bits += __popc(m);
        };
#pragma unroll
        for (int i = 0; i < 8; i++) {
            for (uint32_t r = w[i]; r; r &= r - 1) {
                const int32_t tpos = t0 + 32 * i + (__ffs((int)r) - 1);
                if (one) cell_of((int64_t)u0 + j + kc, tpos, kc, j < 8);
                else {
                    while (kc < M.nch && ce_ < tpos) {
                        kc++; cs_ = cn_;
                        ce_ = kc < M.nch ? M.cend[kc] : 0x7fffffff; cn_ = kc + 1 < M.nch ? M.cstart[kc + 1] : 0x7fffffff;
                    }
                    if (kc < M.nch && cs_ <= tpos) cell_of((int64_t)u0 + j + kc, tpos, kc, false);
                    if (cn_ <= tpos)                              // the chunks behind it that hold tpos too: shared edges
                        for (int64_t kk = kc + 1; kk < M.nch && M.cstart[kk] <= tpos; kk++) cell_of((int64_t)u0 + j + kk, tpos, kk, false);
                }
                j++;
            }
        }
        return bits;
    }
};

// tiletot[workgroup]: the set bits of its tile
__global__ void __launch_bounds__(256) k_mask_count(RankMask M, int per, uint32_t* tiletot) {
    __shared__ int s_w[4];
    const int64_t b0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * per;
    int64_t slot = 0;
    int c = 0;
    for (int k = 0; k < per; k++)
        if (b0 + k < M.X.nblk) { RankBlock B; B.load(M, b0 + k); c += B.walk<false>(M, nullptr, nullptr, 0, slot); }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tiletot[blockIdx.x] = (uint32_t)(s_w[0] + s_w[1] + s_w[2] + s_w[3]);
}

// cap: capacity of cands / keys, *total: the true count, as in k_mask_emit_cells
__global__ void __launch_bounds__(256) k_mask_emit(RankMask M, int per, const uint32_t* tiletot, Cand* cands, uint64_t* keys, int64_t cap,
                                                   unsigned long long* total) {
    __shared__ uint32_t s_p[4];
    __shared__ int s_w[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t front = 0;
    for (int w = threadIdx.x; w < (int)blockIdx.x; w += 256) front += tiletot[w];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) front += __shfl_xor(front, d, 64);
    if (lane == 0) s_p[wv] = front;
    const int64_t b0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * per;
    int64_t slot = 0;
    int c = 0;
    RankBlock B0;                     // the thread's first block stays in registers for the second pass
    for (int k = 0; k < per; k++)
        if (b0 + k < M.X.nblk) {
            RankBlock B;
            B.load(M, b0 + k);
            c += B.walk<false>(M, cands, keys, cap, slot);
            if (k == 0) B0 = B;
        }
    const int incl = wave_incl_add(c, lane);
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    front = s_p[0] + s_p[1] + s_p[2] + s_p[3];
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
        *total = (unsigned long long)front + (unsigned long long)(s_w[0] + s_w[1] + s_w[2] + s_w[3]);
    if (!c) return;
    slot = (int64_t)front + (incl - c);
#pragma unroll
    for (int k = 0; k < 4; k++) if (k < wv) slot += s_w[k];
    for (int k = 0; k < per; k++)
        if (b0 + k < M.X.nblk) {
            RankBlock B = B0;
            if (k > 0) B.load(M, b0 + k);
            B.walk<true>(M, cands, keys, cap, slot);
        }
}

// exclusive prefix sums of a few thousand counts by one workgroup of 1024 threads (the candidate counts of the mask
// tiles), 16 k at a time through LDS: coalesced loads, eight or sixteen consecutive counts per thread, coalesced stores
constexpr int SCAN_SMALL_CHUNK = 16384;
__global__ void __launch_bounds__(1024) k_scan_small(const uint32_t* in, uint32_t* out, int n) {
    __shared__ uint32_t s_v[SCAN_SMALL_CHUNK];
    __shared__ uint32_t s_w[16];
    __shared__ uint32_t s_carry;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    for (int c0 = 0; c0 < n; c0 += SCAN_SMALL_CHUNK) {
        const int m = min(SCAN_SMALL_CHUNK, n - c0);
        for (int i = threadIdx.x; i < m; i += 1024) s_v[i] = in[c0 + i];
        __syncthreads();
        const int per = (m + 1023) / 1024, i0 = (int)threadIdx.x * per;
        uint32_t t = 0;
        for (int k = 0; k < per; k++) if (i0 + k < m) t += s_v[i0 + k];
        uint32_t inc = t;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(inc, d, 64); if (lane >= d) inc += u; }
        if (lane == 63) s_w[wv] = inc;
        __syncthreads();
        uint32_t run = s_carry + inc - t;
        for (int w = 0; w < wv; w++) run += s_w[w];
        for (int k = 0; k < per; k++) if (i0 + k < m) { const uint32_t v = s_v[i0 + k]; s_v[i0 + k] = run; run += v; }
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += 1024) out[c0 + i] = s_v[i];
        if (threadIdx.x == 1023) s_carry = run;          // (the last thread's running sum is the chunk's total + carry)
        __syncthreads();
    }
}

// The kernels behind the candidate count take it from device memory (*n_dev, clamped to the capacity the
// grid was sized for): the host need not have seen it yet.
__device__ __forceinline__ int64_t dev_count(const unsigned long long* n_dev, int64_t cap) {
    const unsigned long long n = *n_dev;
    return n < (unsigned long long)cap ? (int64_t)n : cap;
}

// ---------------------------------------------------------------------------------------
// k_eval_columns: one THREAD per candidate column: walk_column under the chunk's fetch
// rule, genotype_column, is_germ_gt and call_verdict (himut_column.h, caller.py:324-550),
// then under PHASE the haplotype vote where the cascade says PASS (caller.py:552-603).

struct EvalArgs {
    Params P;
    SiteSets S;
    const GtLut* lut;
    const Cand* cands;       // sorted by record key
    int64_t ncand;           // capacity the grid covers; the count itself is *ncand_dev
    const unsigned long long* ncand_dev;
    Reads R;
    Derived D;
    Chunks C;
    Phase H;
    PosIndex X;
    const uint16_t* colstore;
    int64_t nslots;          // capacity of colstore
    himut_record* recs;      // record j belongs to candidate j
    int* err;
};

#ifndef HIMUT_EVAL_WAVES
#define HIMUT_EVAL_WAVES 4
#endif
#ifndef HIMUT_EVAL_BATCH
#define HIMUT_EVAL_BATCH 8
#endif

// The call run's rules for the walk.  keep: only next to the chunk start can a read lie in the pile of the position
// without having been fetched by the chunk (caller.py:299: fetch needs reference_end > chunk_start).  base: under
// PHASE the haplotype vote of the reads that also cover rpos + 1 (caller.py:558-569).
template <bool PHASE>
struct EvalHook {
    const EvalArgs& A;
    const int chunk, ref, alt;
    const int32_t rpos, lo, cs_;
    const bool edge;             // rpos <= the chunk's start
    int32_t tend = 0;            // of the slot's read: keep() leaves it for base()
    uint32_t h0_ref = 0, h1_ref = 0, som0 = 0, som1 = 0;
    __device__ __forceinline__ bool keep(uint32_t i, uint32_t) {
        if (edge || PHASE) {
            tend = A.R.tend[lo + (int32_t)i];
            if (edge && !(tend > cs_)) return false;    // not fetched by this chunk
        }
        return true;
    }
    __device__ __forceinline__ void base(uint32_t i, uint32_t cell, uint32_t) {
        if (!PHASE) return;
        uint32_t hp = HAP_NONE;
        if (tend > rpos + 1 && ((int)cell == ref || (int)cell == alt))
            hp = A.H.hap[A.C.pairoff[chunk] + ((int64_t)(lo + (int32_t)i) - A.C.rlo[chunk])];
        if ((int)cell == ref) { if (hp == HAP_0) h0_ref++; else if (hp == HAP_1) h1_ref++; }   // caller.py:562-564
        if ((int)cell == alt) { if (hp == HAP_0) som0 = 1; else if (hp == HAP_1) som1 = 1; }   // caller.py:565-569
    }
};

template <bool PHASE>
__global__ void __launch_bounds__(256, HIMUT_EVAL_WAVES) k_eval_columns(EvalArgs A) {
    __shared__ double s_lut[3 * 256];
    __shared__ double s_prior[4];
    const int tid = threadIdx.x;
    stage_gt_lut(A.lut, s_lut, s_prior, tid);
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + tid;
    if (j >= dev_count(A.ncand_dev, A.ncand) || *A.err) return;
    const Cand cd = A.cands[j];
    const int32_t tpos = cd.tpos;
    const int chunk = (int)(cd.chunk_bit >> 4);
    const int ref = (int)((cd.chunk_bit >> 2) & 3), alt = (int)(cd.chunk_bit & 3);
    const int32_t rpos = tpos - 1;
    const Column C = column_at(A.X, A.colstore, A.nslots, rpos, pos_rank(A.X, rpos));    // a candidate's position is marked
    if (!C.ok) return;
    const int32_t cs_ = A.C.start[chunk];
    EvalHook<PHASE> hook{A, chunk, ref, alt, rpos, C.lo, cs_, rpos <= cs_};
    Pile pile;
    int bad = 0;
    walk_column<HIMUT_EVAL_BATCH>(C, s_lut, ref, alt, A.P.p.min_bq, hook, pile, bad);
    const Genotyped g = genotype_column(pile, s_prior, ref);

    int status = 255;
    int32_t ps = -1;
    uint32_t flags = 0;
    if (is_germ_gt(g, pile, ref, alt)) flags = REC_GERM;
    else {
        status = call_verdict(A.P, A.S, g, pile, tpos, ref, alt);
        if (PHASE && status == HIMUT_ST_PASS) {  // caller.py:552-603 (unique query names: the voters are the pile's own rows)
            if (!A.P.unique_qnames) {
                // Alignments that share a query name (supplementary alignments: the README asks for -F 0x900, the
                // reference does not insist).  The vote goes by NAME: every alignment over the base behind the
                // candidate (fetch(chrom, tpos, tpos + 1), caller.py:558) whose name is among the names of the
                // column's reference-allele reads votes with ITS haplotype, else one whose name is among the
                // alternative-allele reads' names gives its haplotype to the candidate.
                hook.h0_ref = hook.h1_ref = hook.som0 = hook.som1 = 0;
                const int32_t p1 = rpos + 1;
                const BlockTab b1 = A.X.bt[min((int64_t)(p1 >> 8), A.X.nblk - 1)];
                const uint32_t n1 = b1.ncnt & BT_N_MASK;
                for (uint32_t jj = 0; jj < n1; jj++) {
                    const int64_t jr = (int64_t)b1.lo + jj;
                    if (!(A.R.tstart[jr] <= p1 && A.R.tend[jr] > p1) || (A.D.rflag[jr] & RF_SECONDARY)) continue;
                    const int32_t qj = A.R.qid[jr];
                    bool in_wt = false, in_alt = false;
                    for (uint32_t i = 0; i < C.n; i++) {
                        const uint32_t v = (uint32_t)C.col[(int64_t)i * C.stride];
                        const int cv = (int)(v & 7u);
                        if ((v & 15u) == CELL_EMPTY || (cv != ref && cv != alt)) continue;
                        if (hook.edge && !(A.R.tend[C.lo + (int32_t)i] > cs_)) continue;      // not fetched by this chunk
                        if (A.R.qid[C.lo + (int32_t)i] != qj) continue;
                        if (cv == ref) in_wt = true; else in_alt = true;
                    }
                    if (!in_wt && !in_alt) continue;
                    uint32_t hp = HAP_NONE;       // an alignment the chunk did not fetch spans none of its hetSNPs
                    if (jr >= A.C.rlo[chunk] && jr < A.C.rhi[chunk]) hp = A.H.hap[A.C.pairoff[chunk] + (jr - A.C.rlo[chunk])];
                    if (in_wt) { if (hp == HAP_0) hook.h0_ref++; else if (hp == HAP_1) hook.h1_ref++; }
                    else { if (hp == HAP_0) hook.som0 = 1; else if (hp == HAP_1) hook.som1 = 1; }
                }
            }
            if ((int64_t)hook.h0_ref >= A.P.p.min_hap_count && (int64_t)hook.h1_ref >= A.P.p.min_hap_count && (hook.som0 + hook.som1) == 1)
                ps = cs_;
            else status = HIMUT_ST_UNPHASED;
        }
    }
    pack_record(tpos, chunk, ps, g.gq, ref, alt, g.g0, g.g1, status, g.state, flags, pile.cnt, pile.bqs).store(A.recs + j);
    if (bad) atomicOr(A.err, bad);
}

// ---------------------------------------------------------------------------------------
// finalisation

// som_seen across chunks (caller.py:244,347; bamlib.py:77): a candidate whose tpos was already added by an EARLIER
// chunk is never proposed again.  Whether record i is suppressed: the records of one tpos are neighbours, ordered by
// chunk; a chunk's records are suppressed when a chunk in front of it kept a non-germline candidate there.  Nearly
// every record is alone at its tpos (two key loads); the others replay their group from its head.
__device__ __forceinline__ bool seen_in_earlier_chunk(const himut_record* recs, const uint64_t* keys, int64_t i, int64_t n) {
    const uint64_t tp = keys[i] >> 28;
    const bool first = i == 0 || (keys[i - 1] >> 28) != tp;
    if (first) return false;                       // the group's first chunk (or a record alone) has nothing in front
    const uint64_t mych = (keys[i] >> 4) & 0xffffff;
    int64_t j = i;
    while (j > 0 && (keys[j - 1] >> 28) == tp) j--;
    bool seen = false;
    while (j < n && (keys[j] >> 28) == tp) {
        const uint64_t ch = (keys[j] >> 4) & 0xffffff;
        if (ch == mych) break;
        bool nongerm = false;
        int64_t k = j;
        while (k < n && (keys[k] >> 28) == tp && ((keys[k] >> 4) & 0xffffff) == ch) {
            if (!(recs[k].flags & REC_GERM)) nongerm = true;
            k++;
        }
        if (nongerm) seen = true;
        j = k;
    }
    return seen;
}

// counters (caller.py:625-641) + output flags in sorted order
// emit[] is written for the whole capacity (zeros past the count), so that its scan can run over the capacity.
// Counters: one ballot per counter and wave, one shared-memory add per wave, one global add per block.
// Counter 0 (num_ccs, caller.py:318-320) = the reads the proposals flagged: ccs[0 .. nreads).  Slot 15 of a
// workgroup's partial counters: how many of its records are emitted (k_run_totals turns those into offsets).
__global__ void __launch_bounds__(256) k_finalize_flags(himut_record* recs, const uint64_t* keys, const unsigned long long* n_dev,
                                                        int64_t cap, uint32_t* emit, uint32_t* logpart, const uint8_t* ccs,
                                                        int64_t nreads) {
    __shared__ unsigned int s_log[16];
    if (threadIdx.x < 16) s_log[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    {
        unsigned int f = 0;
        for (int64_t j = i; j < nreads; j += (int64_t)gridDim.x * 256) f += ccs[j];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) f += __shfl_xor(f, d, 64);
        if ((threadIdx.x & 63) == 0 && f) atomicAdd(&s_log[0], f);
    }
    const int64_t n = dev_count(n_dev, cap);
    if (i >= n && i < cap) emit[i] = 0;
    int slot = -1, slot2 = -1;     // the counters this record adds to (besides num_sbs, slot 1)
    bool counted = false, emitted = false;
    if (i < n) {
        himut_record& rec = recs[i];
        uint32_t e = 0;
        const bool suppressed = seen_in_earlier_chunk(recs, keys, i, n);
        if (!suppressed) {
            counted = true;  // num_sbs
            if (rec.flags & REC_GERM) {
                if (rec.gt_state == 1) slot = 2;
                else if (rec.gt_state == 2) slot = 3;
                else if (rec.gt_state == 3) slot = 4;
            } else {
                const int st = rec.status;
                if (st == HIMUT_ST_HET || st == HIMUT_ST_HETALT || st == HIMUT_ST_HOMALT) slot = 5;
                else if (st == HIMUT_ST_INDEL) slot = 7;
                else {
                    slot = 6;  // num_homref_sbs
                    if (st == HIMUT_ST_LOWGQ) slot2 = 8;
                    else if (st == HIMUT_ST_LOWBQ) slot2 = 9;
                    else if (st == HIMUT_ST_PON) slot2 = 10;
                    else if (st == HIMUT_ST_COMSNP) slot2 = 11;
                    else if (st == HIMUT_ST_HIGHDEPTH) slot2 = 12;
                    else if (st == HIMUT_ST_LOWDEPTH) slot2 = 13;
                    else slot2 = 14;  // num_som: PASS and Unphased (caller.py:553,605)
                }
                e = 1;
                if (st == HIMUT_ST_HETALT && i > 0) {
                    // set(): a HetAltSite tuple printed as ref / "a1,a2" is identical for every alt of the column
                    const uint64_t m = ~(uint64_t)3;
                    if ((keys[i - 1] & m) == (keys[i] & m)) {
                        const himut_record& prev = recs[i - 1];
                        // (the neighbour is of this record's tpos and chunk: suppressed or not like this one, i.e. not)
                        if (prev.status == HIMUT_ST_HETALT && !(prev.flags & REC_GERM)) { e = 0; rec.flags |= REC_DUP; }
                    }
                }
            }
        }
        emit[i] = e;
        emitted = e != 0;
    }
    const int lane = threadIdx.x & 63;
    {
        const unsigned long long b = __ballot(counted);
        if (lane == 0 && b) atomicAdd(&s_log[1], (unsigned int)__popcll(b));
        const unsigned long long be = __ballot(emitted);
        if (lane == 0 && be) atomicAdd(&s_log[15], (unsigned int)__popcll(be));
    }
    if (__ballot(slot >= 0 || slot2 >= 0)) {
#pragma unroll
        for (int k = 2; k < 15; k++) {
            const unsigned long long b = __ballot(slot == k || slot2 == k);
            if (lane == 0 && b) atomicAdd(&s_log[k], (unsigned int)__popcll(b));
        }
    }
    __syncthreads();
    // per-workgroup partial counters (one global atomic per workgroup and counter would be ~10^4 atomics on two cache
    // lines, which cost more than the rest of this kernel): the last workgroup adds them up
    if (threadIdx.x < 16) logpart[(int64_t)blockIdx.x * 16 + threadIdx.x] = s_log[threadIdx.x];
}

// The emitted records, in order, to the front of `out`: where a workgroup's records begin comes from k_run_totals
// (wgoff), the place inside the workgroup from wg_rank.
__global__ void __launch_bounds__(256) k_compact(const himut_record* recs, const uint32_t* emit, const uint32_t* wgoff,
                                                 const unsigned long long* n_dev, int64_t cap, himut_record* out) {
    __shared__ int s_w[4];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool e = i < dev_count(n_dev, cap) && emit[i] != 0;
    const WgRank r = wg_rank<4>(e, s_w);
    if (!e) return;
    const uint32_t pos = wgoff[blockIdx.x] + (uint32_t)r.rank;
    const uint4* src = reinterpret_cast<const uint4*>(recs + i);
    uint4 a = src[0], bb = src[1], c = src[2], d = src[3];
    bb.y &= ~REC_W1Y_FLAGS_MASK;  // the flags byte -> 0
    uint4* dst = reinterpret_cast<uint4*>(out + pos);
    dst[0] = a; dst[1] = bb; dst[2] = c; dst[3] = d;
}

// the totals the host reads once at the end of a run: the 15 counters (sums of k_finalize_flags' per-workgroup
// partials), records out and where each workgroup's emitted records begin (the prefix sums of slot 15 of the
// partials), column slots (the end of the last block)
__global__ void __launch_bounds__(1024) k_run_totals(int64_t cap, const uint32_t* blkoff, const uint32_t* blkslots, PosIndex X,
                                                     unsigned long long* nrec, unsigned long long* nslots, const uint32_t* logpart,
                                                     int64_t nparts, unsigned long long* log, uint32_t* wgoff) {
    __shared__ unsigned long long s_log[16];
    __shared__ uint32_t s_w[16];
    if (threadIdx.x < 16) s_log[threadIdx.x] = 0;
    __syncthreads();
    // thread = (row phase, quarter of the 16 counters): 256 rows of partials per pass, 16-byte loads, a few passes
    const int q = threadIdx.x & 3;
    unsigned long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll 4
    for (int64_t b = threadIdx.x >> 2; b < nparts; b += 256) {
        const uint4 v = *reinterpret_cast<const uint4*>(logpart + b * 16 + q * 4);
        a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w;
    }
    // lanes with the same quarter: xor-shuffles over the row-phase bits of the lane index
#pragma unroll
    for (int d = 4; d < 64; d <<= 1) {
        a0 += __shfl_xor(a0, d, 64); a1 += __shfl_xor(a1, d, 64); a2 += __shfl_xor(a2, d, 64); a3 += __shfl_xor(a3, d, 64);
    }
    if ((threadIdx.x & 63) < 4) {
        atomicAdd(&s_log[q * 4 + 0], a0); atomicAdd(&s_log[q * 4 + 1], a1);
        atomicAdd(&s_log[q * 4 + 2], a2); atomicAdd(&s_log[q * 4 + 3], a3);
    }
    // exclusive prefix sums of the workgroups' emitted-record counts
    const int per = (int)((nparts + 1023) / 1024);
    const int64_t p0 = (int64_t)threadIdx.x * per;
    uint32_t t = 0;
    for (int k = 0; k < per; k++) if (p0 + k < nparts) t += logpart[(p0 + k) * 16 + 15];
    uint32_t inc = t;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(inc, d, 64); if (lane >= d) inc += u; }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint32_t run = inc - t;
    for (int w = 0; w < wv; w++) run += s_w[w];
    for (int k = 0; k < per; k++) if (p0 + k < nparts) { wgoff[p0 + k] = run; run += logpart[(p0 + k) * 16 + 15]; }
    if (threadIdx.x < 15) log[threadIdx.x] = s_log[threadIdx.x];
    if (threadIdx.x == 0) {
        *nrec = cap > 0 ? s_log[15] : 0ull;
        *nslots = X.nblk > 0 ? front_totals_of(X, blkoff, blkslots).slots : 0ull;
    }
}

}  // namespace himut
