// The pile tile that k_pile_dense (himut_pile.h) and k_bqcal (himut_bqcal.h) share: TP consecutive positions by the
// rows of the reads that reach them, staged into LDS as cell nibbles and quality bytes, RB rows at a time, for a column
// pass with one thread per position.  __device__ functions and small structs only; each kernel brings what is its own:
// its tile record and tile loop, its fetch rule, its column passes and what it does with a base outside ATGC.
//
//   tile_read_window   the reads that can reach a tile, from two binary searches (k_tile_index, k_bqcal_tiles)
//   pile_list_rows     one round of NT reads of that window: those the kernel's fetch rule keeps, in file order
//   pile_stage_batch   rows [b0, b0 + nb) of the round into LDS: a thread per row turns the read's segments into at most
//                      PILE_MAXP tile pieces, then a wave per row assembles the cells and qualities of the whole row
//   PileTile::cell_at  the cell of row i at tile position x
#pragma once

#include "himut_emit.h"

namespace himut {

constexpr int PILE_MAXP = 4;     // pieces of a row a tile takes before its staging falls back to the segment list

struct PilePiece {   // the part of one gapless segment (or deletion) of a read inside the tile: tile-local [x0, x1), query offset of x0
    int32_t x0, x1;
    int32_t qa;
    uint32_t flags;  // SEG_DEL, SEG_INS (insertion in front of position x0)
};

// The LDS of a tile of TP positions, RB rows per batch, for a workgroup of NT threads.
template <int TP, int RB, int NT>
struct PileTile {
    static constexpr int PPL = TP / 64;        // positions per lane when a wave stages one row
    static constexpr int NW = NT / 64;
    static_assert(PPL == 8, "a lane stages eight positions of a row: the tile is 512 wide");
    alignas(16) uint8_t bq[RB * TP];
    alignas(16) uint8_t cell[RB * TP / 2];
    alignas(16) PilePiece piece[RB * PILE_MAXP];
    int64_t rowqo[RB];
    int rowread[RB];
    uint8_t rownp[RB];
    uint16_t rows[NT];
    int wcnt[NW];

    __device__ __forceinline__ uint32_t cell_at(int i, int x) const { return (cell[i * (TP / 2) + (x >> 1)] >> (4 * (x & 1))) & 15; }
};

// The window of the reads [rlo, rhi) that can reach the tile [p0, p1): those with tstart < p1, from the first one at
// which the running maximum of tend is >= p0.
__device__ __forceinline__ void tile_read_window(const Reads& R, int64_t rlo, int64_t rhi, int32_t p0, int32_t p1, int64_t& lo, int32_t& nwin) {
    const int64_t hi = lower_bound(R.tstart, rlo, rhi, p1);
    lo = lower_bound(R.prefmax_tend, rlo, hi, p0);
    nwin = (int32_t)(hi - lo);
}

// One round of the window: thread tid has looked at read base + tid and says whether the tile takes it (ok).  Leaves
// the kept threads in L.rows, in file order (wg_rank, himut_emit.h), and returns how many there are.  Two workgroup
// barriers, for every thread: wg_rank's and one behind the list.
template <int TP, int RB, int NT>
__device__ __forceinline__ int pile_list_rows(PileTile<TP, RB, NT>& L, const bool ok) {
    const WgRank r = wg_rank<NT / 64>(ok, L.wcnt);
    if (ok) L.rows[r.rank] = (uint16_t)threadIdx.x;
    __syncthreads();
    return r.total;
}

// Rows [b0, b0 + nb) of the round that starts at read `base` (nb <= RB) into L.cell and L.bq, rows [0, nb), for the
// tile [p0, p1); lo: the first read of the tile's window.  Returns whether a base cell this thread staged from a piece
// is outside ATGC.  Two workgroup barriers, for every thread: behind the row setup and behind the staging.
template <int TP, int RB, int NT>
__device__ __forceinline__ bool pile_stage_batch(PileTile<TP, RB, NT>& L, const Reads& R, const Derived& D, const int64_t base, const int64_t lo,
                                                 const int b0, const int nb, const int32_t p0, const int32_t p1) {
    constexpr int PPL = PileTile<TP, RB, NT>::PPL, NW = PileTile<TP, RB, NT>::NW, MAXP = PILE_MAXP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bool other = false;
    // ---- row setup: one thread per row turns the read's segments into tile pieces
    if (tid < nb) {
        const int64_t rr = base + L.rows[b0 + tid];
        const int ns = D.nseg[rr];
        const Seg* segs = D.segs + seg_base(R, rr);
        L.rowqo[tid] = R.qoff[rr];
        L.rowread[tid] = (int)(rr - lo);
        int np = 0;
        // the segments are sorted and do not overlap, and only a trailing insertion has no length: the walk starts at
        // the one that holds p0 (or the last one in front of it), found in log2(ns) loads -- a read's text splits into
        // tens of segments and a walk from its first one is as many dependent loads
        int j = 0;
        for (int hi = ns; j < hi;) {
            const int m = (j + hi) >> 1;
            if (segs[m].t0 <= p0) j = m + 1; else hi = m;
        }
        for (j = max(j - 1, 0); j < ns; j++) {
            const Seg sg = segs[j];
            if (sg.t0 >= p1) break;
            const int32_t eend = sg.t0 + ((sg.flags & SEG_INS) ? max(sg.len, 1) : sg.len);
            if (eend <= p0) continue;
            if (np < MAXP) {
                PilePiece pc;
                pc.x0 = max(sg.t0, p0) - p0;
                pc.x1 = max(min(sg.t0 + sg.len, p1) - p0, pc.x0);
                pc.qa = sg.q0 + (p0 + pc.x0 - sg.t0);
                pc.flags = (sg.flags & SEG_DEL) | (((sg.flags & SEG_INS) && sg.t0 >= p0) ? SEG_INS : 0u);
                L.piece[tid * MAXP + np] = pc;
            }
            np++;
        }
        L.rownp[tid] = (uint8_t)min(np, 255);
    }
    __syncthreads();
    // ---- staging: one wave per row; every lane assembles its PPL positions in registers
    for (int i = wave; i < nb; i += NW) {
        const int gx = lane * PPL;
        uint64_t cell = 0x7777777777777777ULL;  // CELL_EMPTY everywhere (low PPL nibbles used)
        uint64_t bqw = 0;
        const int np = L.rownp[i];
        const int64_t qo = L.rowqo[i];
        if (np <= MAXP) {
            for (int k = 0; k < np; k++) {
                const PilePiece pc = L.piece[i * MAXP + k];
                const int a = max(pc.x0, gx) - gx, b = min(pc.x1, gx + PPL) - gx;
                if ((pc.flags & SEG_INS) && pc.x0 >= gx && pc.x0 < gx + PPL) cell |= 8ULL << (4 * (pc.x0 - gx));
                const bool cov = a < b;
                const int aa = cov ? a : 0, bb = cov ? b : 0;
                const uint64_t nm = ((1ULL << (4 * bb)) - 1ULL) & ~((1ULL << (4 * aa)) - 1ULL);  // nibbles [a, b)
                if (pc.flags & SEG_DEL) {
                    cell = (cell & ~(nm & 0x7777777777777777ULL)) | (nm & 0x5555555555555555ULL);
                } else {
                    // loads are issued unconditionally (clamped address) so that they go out together
                    const int64_t o = qo + pc.qa + (cov ? (gx + a - pc.x0) : 0);
                    const uint8_t* sp = R.seq + (o >> 1);
                    uint32_t w32;
                    __builtin_memcpy(&w32, sp, 4);
                    const uint32_t extra = sp[4];
                    uint64_t l;
                    __builtin_memcpy(&l, R.bq + o, 8);
                    uint64_t w = w32;
                    w = ((w & 0x0f0f0f0f0f0f0f0fULL) << 4) | ((w >> 4) & 0x0f0f0f0f0f0f0f0fULL);
                    if (o & 1) w = (w >> 4) | ((uint64_t)(extra >> 4) << 28);
                    const uint64_t codes = nib16_to_cells(w) << (4 * aa);
                    if (codes & nm & 0x4444444444444444ULL) other = true;      // CELL_OTHER
                    cell = (cell & ~(nm & 0x7777777777777777ULL)) | (codes & nm);
                    const uint64_t bm = ((bb >= 8) ? ~0ULL : ((1ULL << (8 * bb)) - 1ULL)) & ~((1ULL << (8 * aa)) - 1ULL);
                    bqw |= (l << (8 * aa)) & bm;
                }
            }
        } else {
            // rare: more than MAXP pieces in one tile -> position by position from the segment list
            const int64_t rr = lo + L.rowread[i];
            const Seg* segs = D.segs + seg_base(R, rr);
            const int ns = D.nseg[rr];
            for (int j = 0; j < PPL; j++) {
                const int32_t pp = p0 + gx + j;
                for (int q = 0; q < ns; q++) {
                    const Seg sg = segs[q];
                    if (sg.t0 > pp) break;
                    if (pp == sg.t0 && (sg.flags & SEG_INS)) cell |= 8ULL << (4 * j);
                    if (pp < sg.t0 + sg.len) {
                        uint64_t code;
                        if (sg.flags & SEG_DEL) code = CELL_DEL;
                        else {
                            const int64_t o = qo + sg.q0 + (pp - sg.t0);
                            code = (uint64_t)nib2allele(nib_at(R.seq, o));
                            bqw |= (uint64_t)R.bq[o] << (8 * j);
                        }
                        cell = (cell & ~(7ULL << (4 * j))) | (code << (4 * j));
                    }
                }
            }
        }
        *reinterpret_cast<uint32_t*>(&L.cell[i * (TP / 2) + lane * 4]) = (uint32_t)cell;
        *reinterpret_cast<uint64_t*>(&L.bq[i * TP + lane * 8]) = bqw;
    }
    __syncthreads();
    return other;
}

}  // namespace himut
