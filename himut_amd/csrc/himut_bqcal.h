// Device code of the bqcal run (himut_run_bqcal): every position of the regions genotyped, every pile base of a
// confidently genotyped column binned by its reported quality.  The contract is include/himut_hip.h's (DESIGN section 8,
// Row 8).  Behind the read pass every pipeline starts with (k_parse_cs) the run has four kernels of its own:
//
//   k_bqcal_bases    sixteen lanes per read: a flagged read (k_flag_bases) that some region fetches is looked at base
//                    by base (HIMUT_ERR_BASE, the germline run's rule)
//   k_bqcal_tiles    one thread per tile of BQ_TP positions of a region: its positions and its window of reads
//   k_bqcal          a grid of resident workgroups, each looping over tiles in xcd_remap order.  Per tile the pile rows
//                    are staged into LDS by the pile tile of himut_piletile.h, which k_pile_dense runs on too (the row
//                    listing, a thread per row for its pieces, a wave per row for its cell nibbles and quality bytes),
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

#include "himut_piletile.h"

namespace himut {

// tile width, LDS row batch (the most), threads
constexpr int BQ_TP = 512, BQ_RB = 64, BQ_NT = 512;
constexpr int BQ_ROW = 2 * 256 + 12;          // a partial row: match[256], mismatch[256], log[12]
constexpr int BQ_FLUSH_TILES = 256;           // a wave's bin takes 64 positions x the tile's rows per tile: below 2^32 up to 2^18 rows

struct BqTile {
    int32_t p0;      // first position
    int32_t npos;    // positions
    int32_t nwin;    // reads in the window [lo, lo + nwin)
    int32_t pad;
    int64_t lo;
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
    tile_read_window(R, 0, R.n, t.p0, p1, t.lo, t.nwin);
    t.pad = 0;
    out[tile] = t;
}

__global__ void __launch_bounds__(BQ_NT, 4) k_bqcal(BqArgs A) {
    constexpr int TP = BQ_TP, NT = BQ_NT, RB = BQ_RB;
    constexpr int NW = NT / 64;
    static_assert(NT == TP, "a thread owns one position of the tile");
    // One block, so that the order is the kernel's and not the compiler's.  The LUT lies behind the first 64 KB on a
    // 2 KB boundary: a cell's three table entries are 2 KB apart, and there the column walk reads them with three
    // ds_read_b64 on addresses of their own.  In front of 64 KB the compiler folds two of them into one
    // ds_read2st64_b64, which costs the run 1.2 % (Row 8).
    struct Lds {
        PileTile<TP, RB, NT> tile;
        uint32_t hist[NW][2][256];            // per wave: match, mismatch
        double prior[4];
        uint32_t log[12];
        alignas(2048) double lut[3 * 256];
    };
    static_assert(offsetof(Lds, lut) >= 65536, "the LUT behind the first 64 KB of LDS");
    __shared__ Lds s_lds;
    PileTile<TP, RB, NT>& s_tile = s_lds.tile;
    uint32_t (&s_hist)[NW][2][256] = s_lds.hist;
    double* const s_lut = s_lds.lut;
    double* const s_prior = s_lds.prior;
    uint32_t* const s_log = s_lds.log;

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
                    const uint32_t cb = s_tile.cell_at(i, x);
                    if (cb == CELL_EMPTY) continue;
                    if (cb & CELL_INS) nins++;
                    const int a = cb & 7;
                    if (a < 4) {
                        const uint32_t q = s_tile.bq[i * TP + x];
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
                    const uint32_t cb = s_tile.cell_at(i, x);
                    const int a = cb & 7;
                    if (cb == CELL_EMPTY || a >= 4) continue;
                    if (mode == 2 && ((gtmask >> a) & 1u)) continue;      // the genotype's own cells at a mismatch position: nowhere
                    const int q = s_tile.bq[i * TP + x];
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
                const int nrows = pile_list_rows(s_tile, ok);

                for (int b0 = 0; b0 < nrows; b0 += rb) {
                    const int nb = min(rb, nrows - b0);
                    pile_stage_batch(s_tile, R, D, base, T.lo, b0, nb, p0, p1);      // a base outside ATGC: k_bqcal_bases' rule
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
