// Device code of the dense pile (himut_pile_counts, himut_pile.hip): counts + BQ sums for EVERY position of a range.
//
//   k_tile_index / k_pile_dense
//                      one workgroup per tile of PD_TP positions, over the pile tile of himut_piletile.h (the tile's read
//                      window, the row listing, the LDS staging of cells and qualities), which k_bqcal stages its rows
//                      with too
#pragma once

#include "himut_piletile.h"

namespace himut {

// ---------------------------------------------------------------------------------------
// k_pile_dense: counts + BQ sums at every position of the given chunks, through
// LDS-staged base / BQ tiles (one workgroup per PD_TP positions; the staging: himut_piletile.h).

struct TileInfo {
    int32_t chunk;
    int32_t p0;     // first rpos of the tile
    int32_t npos;   // positions in the tile
    int32_t nwin;   // reads in the candidate window [lo, lo + nwin)
    int64_t lo;
    int64_t outbase;  // index of the tile's first position in the output arrays
};

template <int TP>
__global__ void __launch_bounds__(256) k_tile_index(Reads R, Chunks C, const int64_t* tileoff, int64_t n_tiles, TileInfo* out) {
    const int64_t tile = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tile >= n_tiles) return;
    const int64_t c = upper_bound(tileoff, (int64_t)0, C.n + 1, tile) - 1;
    const int32_t cs_ = C.start[c], ce_ = C.end[c];
    const int64_t local = (tile - tileoff[c]) * TP;
    TileInfo t;
    t.chunk = (int32_t)c;
    t.p0 = (int32_t)(cs_ - 1 + local);
    const int32_t p1 = (int32_t)min((int64_t)t.p0 + TP, (int64_t)ce_);  // last rpos of the chunk is end - 1
    t.npos = p1 - t.p0;
    tile_read_window(R, C.rlo[c], C.rhi[c], t.p0, p1, t.lo, t.nwin);
    t.outbase = C.maskoff[c] + local;
    out[tile] = t;
}

struct DenseArgs {
    Reads R;
    Derived D;
    Chunks C;
    const TileInfo* tiles;
    int64_t n_tiles;
    uint32_t* counts;  // [position][6]
    uint32_t* bqsum;   // [position][4]
    int* err;
};

template <int TP, int RB, int NT>
__global__ void __launch_bounds__(NT) k_pile_dense(DenseArgs A) {
    constexpr int DPT = TP / NT;        // positions per thread in the column pass
    __shared__ PileTile<TP, RB, NT> s_tile;

    const int tid = threadIdx.x;
    const Reads& R = A.R;
    const Derived& D = A.D;
    const TileInfo T = A.tiles[xcd_remap(blockIdx.x, A.n_tiles)];
    const int32_t p0 = T.p0, p1 = T.p0 + T.npos;
    const int32_t cs_ = A.C.start[T.chunk], ce_ = A.C.end[T.chunk];

    uint32_t dcnt[DPT][6];
    uint32_t dbq[DPT][4];
#pragma unroll
    for (int d = 0; d < DPT; d++) {
#pragma unroll
        for (int k = 0; k < 6; k++) dcnt[d][k] = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) dbq[d][k] = 0;
    }
    int bad = 0;

    for (int64_t base = T.lo; base < T.lo + T.nwin; base += NT) {
        // ---- rows of the tile, in fetch order (fetch rule of the chunk: caller.py:299)
        const int64_t r = base + tid;
        bool ok = false;
        if (r < T.lo + T.nwin) {
            const int32_t te = R.tend[r];
            ok = !(D.rflag[r] & RF_SECONDARY) && te >= p0 && te > cs_ && R.tstart[r] < ce_;
        }
        const int nrows = pile_list_rows(s_tile, ok);

        for (int b0 = 0; b0 < nrows; b0 += RB) {
            const int nb = min(RB, nrows - b0);
            if (pile_stage_batch(s_tile, R, D, base, T.lo, b0, nb, p0, p1)) bad |= 1 << HIMUT_ERR_BASE;  // caller.py:57
            // ---- column pass: thread = position, rows in fetch order
#pragma unroll
            for (int d = 0; d < DPT; d++) {
                const int x = tid + d * NT;
                if (x < T.npos) {
                    for (int i = 0; i < nb; i++) {
                        const uint32_t cb = s_tile.cell_at(i, x);
                        if (cb == CELL_EMPTY) continue;
                        if (cb & CELL_INS) dcnt[d][4]++;
                        const int a = cb & 7;
                        if (a < 4) {
                            const uint32_t q = s_tile.bq[i * TP + x];
#pragma unroll
                            for (int b = 0; b < 4; b++) if (a == b) { dcnt[d][b]++; dbq[d][b] += q; }
                        } else if (a == CELL_DEL) dcnt[d][5]++;
                        else if (a == CELL_OTHER) bad |= 1 << HIMUT_ERR_BASE;
                    }
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int d = 0; d < DPT; d++) {
        const int x = tid + d * NT;
        if (x < T.npos) {
            const int64_t o = T.outbase + x;
#pragma unroll
            for (int k = 0; k < 6; k++) A.counts[o * 6 + k] = dcnt[d][k];
#pragma unroll
            for (int k = 0; k < 4; k++) A.bqsum[o * 4 + k] = dbq[d][k];
        }
    }
    if (bad) atomicOr(A.err, bad);
}

}  // namespace himut
