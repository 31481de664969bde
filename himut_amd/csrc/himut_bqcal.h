// Device code of the bqcal run (himut_run_bqcal): every position of the regions genotyped, every pile base of a
// confidently genotyped column binned by its reported quality.  The contract is include/himut_hip.h's (DESIGN section 8,
// Row 8).  Behind the read pass every pipeline starts with (k_parse_cs) the run has four kernels of its own:
//
//   k_bqcal_bases    sixteen lanes per read: a flagged read (k_flag_bases) that some region fetches is looked at base
//                    by base (HIMUT_ERR_BASE, the germline run's rule)
//   k_bqcal_tiles    one thread per tile of BQ_TP positions of a region: its positions and its window of reads
//   k_bqcal          a grid of resident workgroups, each looping over tiles in xcd_remap order.  Per tile the pile rows
//                    are staged into LDS as k_pile_dense stages them (a wave per row: cell nibbles and quality bytes),
//                    BQ_RB rows at a time, and one THREAD per position walks them in fetch order: counts and the three
//                    ordered fp64 sums per allele.  The verdict needs the whole column -- the skips, genotype(), the
//                    set of alleles that count as matches -- so the bases are binned in a second walk over the same
//                    LDS rows; a tile with more rows than one batch stages its batches again for it.  A thread bins
//                    runs, not cells: consecutive rows of a column mostly share their quality, and a run costs one LDS
//                    add into its wave's own pair of histograms.  The counters are one ballot per wave and counter.
//                    Nothing goes to global memory per tile: a workgroup adds its histograms and counters to its own
//                    partial row (at its end, and every BQ_FLUSH_TILES tiles so that no 32-bit bin can wrap)
//   k_bqcal_reduce   the partial rows summed, one thread per bin
#pragma once

#include "himut_device.h"

namespace himut {

// tile width, LDS row batch (the most), threads, pieces of a row a tile takes before it falls back to the segment list
constexpr int BQ_TP = 512, BQ_RB = 64, BQ_NT = 512, BQ_MAXP = 4;
constexpr int BQ_ROW = 2 * 256 + 12;          // a partial row: match[256], mismatch[256], log[12]
constexpr int BQ_FLUSH_TILES = 256;           // a wave's bin takes 64 positions x the tile's rows per tile: below 2^32 up to 2^18 rows

struct BqTile {
    int32_t p0;      // first position
    int32_t npos;    // positions
    int32_t nwin;    // reads in the window [lo, lo + nwin)
    int32_t pad;
    int64_t lo;
};

struct BqPiece {     // the part of one gapless segment (or deletion) of a read inside the tile: tile-local [x0, x1), query offset of x0
    int32_t x0, x1;
    int32_t qa;
    uint32_t flags;  // SEG_DEL, SEG_INS (insertion in front of position x0)
};

struct BqArgs {
    himut_bqcal_params p;
    const GtLut* lut;
    Reads R;
    Derived D;
    const uint8_t* refseq;
    const BqTile* tiles;
    int64_t n_tiles;
    int rb;                      // rows per LDS batch, 1 .. BQ_RB
    unsigned long long* part;    // BQ_ROW sums per workgroup, zero on entry
    int* err;
};

// the reads some region fetches (s < tend and e > tstart; starts ascending, the running maximum of their ends)
__global__ void __launch_bounds__(256) k_bqcal_bases(Reads R, Derived D, const int32_t* s_start, const int32_t* s_pmaxend, int64_t nregion,
                                                     int* err) {
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int gl = threadIdx.x & 15;
    if (r >= R.n || !R.nonacgt[r] || (D.rflag[r] & RF_SECONDARY)) return;
    const ReadMeta M = D.meta[r];
    if (M.nseg <= 0) return;
    const int64_t k = lower_bound(s_start, (int64_t)0, nregion, M.tend);         // regions with start < tend
    if (k > 0 && s_pmaxend[k - 1] > M.tstart && !aligned_bases_ok(R, D.segs + M.segbase, M.nseg, M.qoff, gl, 16))
        set_err(err, HIMUT_ERR_BASE);
}

// tileoff: n_regions + 1 entries, the regions' first tiles
__global__ void __launch_bounds__(256) k_bqcal_tiles(Reads R, const int32_t* rstart, const int32_t* rend, const int64_t* tileoff,
                                                     int64_t n_regions, int64_t n_tiles, BqTile* out) {
    const int64_t tile = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tile >= n_tiles) return;
    const int64_t c = upper_bound(tileoff, (int64_t)0, n_regions + 1, tile) - 1;
    BqTile t;
    t.p0 = (int32_t)((int64_t)rstart[c] + (tile - tileoff[c]) * BQ_TP);
    const int32_t p1 = (int32_t)min((int64_t)t.p0 + BQ_TP, (int64_t)rend[c]);
    t.npos = p1 - t.p0;
    const int64_t hi = lower_bound(R.tstart, (int64_t)0, R.n, p1);                // reads with tstart < p1
    t.lo = lower_bound(R.prefmax_tend, (int64_t)0, hi, t.p0);                     // running max of tend >= p0
    t.nwin = (int32_t)(hi - t.lo);
    t.pad = 0;
    out[tile] = t;
}

__global__ void __launch_bounds__(BQ_NT, 4) k_bqcal(BqArgs A) {
    constexpr int TP = BQ_TP, NT = BQ_NT, RB = BQ_RB, MAXP = BQ_MAXP;
    constexpr int PPL = TP / 64;        // positions per lane when a wave stages one row
    constexpr int NW = NT / 64;
    static_assert(PPL == 8 && NT == TP, "a lane stages eight positions of a row; a thread owns one position of the tile");
    __shared__ double s_lut[3 * 256];
    __shared__ double s_prior[4];
    __shared__ __align__(16) uint8_t s_bq[RB * TP];
    __shared__ __align__(16) uint8_t s_cell[RB * TP / 2];
    __shared__ __align__(16) BqPiece s_piece[RB * MAXP];
    __shared__ int64_t s_rowqo[RB];
    __shared__ int s_rowread[RB];
    __shared__ uint8_t s_rownp[RB];
    __shared__ uint16_t s_rows[NT];
    __shared__ int s_wcnt[NW];
    __shared__ uint32_t s_hist[NW][2][256];   // per wave: match, mismatch
    __shared__ uint32_t s_log[12];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Reads& R = A.R;
    const Derived& D = A.D;
    for (int i = tid; i < 3 * 256; i += NT) s_lut[i] = A.lut->t[i >> 8][i & 255];
    if (tid < 4) s_prior[tid] = A.lut->prior[tid];
    for (int i = tid; i < NW * 2 * 256; i += NT) (&s_hist[0][0][0])[i] = 0;
    if (tid < 12) s_log[tid] = 0;
    __syncthreads();
    const int rb = A.rb;
    const int min_mapq = A.p.min_mapq;
    unsigned long long* const part = A.part + (int64_t)blockIdx.x * BQ_ROW;
    // the workgroup's histograms and counters into its partial row (nobody else's), and empty again
    auto flush = [&]() {
        __syncthreads();
        {
            unsigned long long s = 0;
#pragma unroll
            for (int w = 0; w < NW; w++) { s += s_hist[w][tid >> 8][tid & 255]; s_hist[w][tid >> 8][tid & 255] = 0; }
            if (s) part[tid] += s;
        }
        if (tid < 12) { if (s_log[tid]) part[512 + tid] += s_log[tid]; s_log[tid] = 0; }
        __syncthreads();
    };
    int bad = 0;
    int since_flush = 0;

    for (int64_t tl = blockIdx.x; tl < A.n_tiles; tl += gridDim.x) {
        const BqTile T = A.tiles[xcd_remap(tl, A.n_tiles)];
        const int32_t p0 = T.p0, p1 = T.p0 + T.npos;
        const int x = tid;
        const bool mine = x < T.npos;
        // step 1 needs no pile: a thread whose letter is not one of ACGT walks no column
        const int ref = mine ? char2allele((int)A.refseq[p0 + x]) : -1;
        uint32_t cnt[4] = {0, 0, 0, 0}, nins = 0, ndel = 0, ref_count = 0;
        bool q0 = false;
        GtSums S;
#pragma unroll
        for (int b = 0; b < 4; b++) { S[0][b] = 0.0; S[1][b] = 0.0; S[2][b] = 0.0; }
        double R0 = 0.0, R1 = 0.0, R2 = 0.0;      // the reference allele's three sums: nearly every cell
        int mode = 0;                             // behind the verdict: 1 every base cell is a match, 2 the cells outside gtmask are mismatches
        uint32_t gtmask = 0;
        int cur = 0;                              // the run of equal qualities the binning walk is in
        uint32_t run = 0;
        int nbat = 0, one_nb = 0;                 // batches of the first walk; the rows of the last one

        // the thread's column over rows [0, nb) of the batch in LDS: first walk the sums, second walk the bins
        auto column = [&](int nb, int pass) {
            if (pass == 0) {
                if (ref < 0) return;
                for (int i = 0; i < nb; i++) {
                    const uint32_t cb = (s_cell[i * (TP / 2) + (x >> 1)] >> (4 * (x & 1))) & 15;
                    if (cb == CELL_EMPTY) continue;
                    if (cb & CELL_INS) nins++;
                    const int a = cb & 7;
                    if (a < 4) {
                        const uint32_t q = s_bq[i * TP + x];
                        if (q == 0) q0 = true;
                        const double vh = s_lut[q], vt = s_lut[256 + q], ve = s_lut[512 + q];
                        if (a == ref) {
                            ref_count++;
                            R0 = R0 + vh; R1 = R1 + vt; R2 = R2 + ve;
                        } else {
#pragma unroll
                            for (int b = 0; b < 4; b++) {
                                if (a == b) {
                                    cnt[b]++;
                                    S[0][b] = S[0][b] + vh;
                                    S[1][b] = S[1][b] + vt;
                                    S[2][b] = S[2][b] + ve;
                                }
                            }
                        }
                    } else if (a == CELL_DEL) ndel++;
                }
            } else {
                if (mode == 0) return;
                uint32_t* h = s_hist[wave][mode - 1];
                for (int i = 0; i < nb; i++) {
                    const uint32_t cb = (s_cell[i * (TP / 2) + (x >> 1)] >> (4 * (x & 1))) & 15;
                    const int a = cb & 7;
                    if (cb == CELL_EMPTY || a >= 4) continue;
                    if (mode == 2 && ((gtmask >> a) & 1u)) continue;      // the genotype's own cells at a mismatch position: nowhere
                    const int q = s_bq[i * TP + x];
                    if (q == cur) run++;
                    else {
                        if (run) atomicAdd(&h[cur], run);
                        cur = q; run = 1;
                    }
                }
            }
        };

        for (int pass = 0; pass < 2; pass++) {
            if (pass == 1) {
                // ---- the verdict of the thread's position, and the tile's counters
                int cat = 0;                  // the log slot of the position: 1-4 skipped at that step, 5-8 passed with that state
                if (mine) {
#pragma unroll
                    for (int b = 0; b < 4; b++)
                        if (b == ref) { cnt[b] = ref_count; S[0][b] = R0; S[1][b] = R1; S[2][b] = R2; }
                    const uint32_t nbase = cnt[0] + cnt[1] + cnt[2] + cnt[3];
                    if (ref < 0) cat = 1;
                    else if ((int64_t)nbase + ndel >= (int64_t)A.p.md_threshold) cat = 2;
                    else if (nins != 0 || ndel != 0) cat = 3;
                    else {
                        if (q0) bad |= 1 << HIMUT_ERR_BQ0;                     // gtlib.py:64
                        const Genotype gt = genotype(S, s_prior, ref);
                        if (gt.gq < A.p.min_gq) cat = 4;
                        else {
                            const int g0 = (int)HIMUT_GT_B1(gt.best), g1 = (int)HIMUT_GT_B2(gt.best);
                            cat = 5 + gt_state_of(g0, g1, ref);
                            gtmask = (1u << g0) | (1u << g1);
                            uint32_t inside = 0;
#pragma unroll
                            for (int b = 0; b < 4; b++) if ((gtmask >> b) & 1u) inside += cnt[b];
                            mode = inside != nbase ? 2 : (nbase ? 1 : 0);
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < 11; k++) {
                    const bool in = k == 0 ? mine : k == 9 ? mode == 1 : k == 10 ? mode == 2 : cat == k;
                    const int n = (int)__popcll(__ballot(in));
                    if (lane == 0 && n) atomicAdd(&s_log[k], (uint32_t)n);
                }
                if (!__syncthreads_or(mode != 0)) break;                       // nothing of the tile is binned
                if (nbat == 1) {                                               // the tile's only batch is still in LDS
                    column(one_nb, 1);
                    break;
                }
            }
            for (int64_t base = T.lo; base < T.lo + T.nwin; base += NT) {
                // ---- rows of the tile, in file order
                const int64_t r = base + tid;
                bool ok = false;
                if (r < T.lo + T.nwin)
                    ok = !(D.rflag[r] & RF_SECONDARY) && (int)R.mapq[r] >= min_mapq && R.tend[r] >= p0 && R.tstart[r] < p1;
                const unsigned long long bal = __ballot(ok);
                if (lane == 0) s_wcnt[wave] = __popcll(bal);
                __syncthreads();
                int woff = 0, nrows = 0;
#pragma unroll
                for (int k = 0; k < NW; k++) { if (k < wave) woff += s_wcnt[k]; nrows += s_wcnt[k]; }
                if (ok) s_rows[woff + __popcll(bal & ((1ULL << lane) - 1ULL))] = (uint16_t)tid;
                __syncthreads();

                for (int b0 = 0; b0 < nrows; b0 += rb) {
                    const int nb = min(rb, nrows - b0);
                    // ---- row setup: one thread per row turns the read's segments into tile pieces
                    if (tid < nb) {
                        const int64_t rr = base + s_rows[b0 + tid];
                        const int ns = D.nseg[rr];
                        const Seg* segs = D.segs + seg_base(R, rr);
                        s_rowqo[tid] = R.qoff[rr];
                        s_rowread[tid] = (int)(rr - T.lo);
                        int np = 0;
                        // the segments are sorted and do not overlap: the walk starts at the one that holds p0 (or the last one in
                        // front of it), found in log2(ns) loads -- a read's text splits into tens of segments and a walk
                        // from its first one is as many dependent loads
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
                                BqPiece pc;
                                pc.x0 = max(sg.t0, p0) - p0;
                                pc.x1 = max(min(sg.t0 + sg.len, p1) - p0, pc.x0);
                                pc.qa = sg.q0 + (p0 + pc.x0 - sg.t0);
                                pc.flags = (sg.flags & SEG_DEL) | (((sg.flags & SEG_INS) && sg.t0 >= p0) ? SEG_INS : 0u);
                                s_piece[tid * MAXP + np] = pc;
                            }
                            np++;
                        }
                        s_rownp[tid] = (uint8_t)min(np, 255);
                    }
                    __syncthreads();
                    // ---- staging: one wave per row; every lane assembles its PPL positions in registers
                    for (int i = wave; i < nb; i += NW) {
                        const int gx = lane * PPL;
                        uint64_t cell = 0x7777777777777777ULL;  // CELL_EMPTY everywhere (low PPL nibbles used)
                        uint64_t bqw = 0;
                        const int np = s_rownp[i];
                        const int64_t qo = s_rowqo[i];
                        if (np <= MAXP) {
                            for (int k = 0; k < np; k++) {
                                const BqPiece pc = s_piece[i * MAXP + k];
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
                                    cell = (cell & ~(nm & 0x7777777777777777ULL)) | (codes & nm);
                                    const uint64_t bm = ((bb >= 8) ? ~0ULL : ((1ULL << (8 * bb)) - 1ULL)) & ~((1ULL << (8 * aa)) - 1ULL);
                                    bqw |= (l << (8 * aa)) & bm;
                                }
                            }
                        } else {
                            // rare: more than MAXP pieces in one tile -> position by position from the segment list
                            const int64_t rr = T.lo + s_rowread[i];
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
                        *reinterpret_cast<uint32_t*>(&s_cell[i * (TP / 2) + lane * 4]) = (uint32_t)cell;
                        *reinterpret_cast<uint64_t*>(&s_bq[i * TP + lane * 8]) = bqw;
                    }
                    __syncthreads();
                    // ---- column walk: thread = position, rows in fetch order
                    if (mine) column(nb, pass);
                    if (pass == 0) { nbat++; one_nb = nb; }
                    __syncthreads();
                }
            }
        }
        if (run) atomicAdd(&s_hist[wave][mode - 1][cur], run);
        if (++since_flush == BQ_FLUSH_TILES) { flush(); since_flush = 0; }
        else __syncthreads();           // the next tile's rows overwrite what this tile's walk reads
    }
    flush();
    if (bad) atomicOr(A.err, bad);
}

// out[j] = the sum of the partial rows' j-th entries
__global__ void __launch_bounds__(256) k_bqcal_reduce(const unsigned long long* part, int64_t nrows, long long* out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= BQ_ROW) return;
    unsigned long long s = 0;
    for (int64_t w = 0; w < nrows; w++) s += part[w * BQ_ROW + j];
    out[j] = (long long)s;
}

}  // namespace himut
