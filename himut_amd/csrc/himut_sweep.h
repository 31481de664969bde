// What the normcounts sweep's kernels and the callable run's map sweep share (himut_norm.h, himut_normq.h,
// himut_callmap.h): the kernels' arguments, the state of one position and its classification (normcounts.py:243-402;
// gtlib.py:72-174 for the sums), and the tile sweep -- a workgroup's 256 positions of a chunk, the cells of the reads
// over them built in LDS 48 rows at a time, every thread down its column.
//
//   NormArgs                        the arguments
//   NormPos                         a position's counts and sums; the column walk's update; the 16-bit fields
//   norm_classify, norm_tally       the verdict of a position (k_norm_tile, k_norm_dirty, k_callmap_sweep), and what it
//                                   adds to the counters and the trinucleotide bins
//   NormTally, NormLds              a workgroup's counters; with the tables and the cells of the tile sweep
//   norm_tile_at, norm_sweep_tile   a tile of a chunk; its rows built (norm_build_rows) and walked (norm_walk_columns)
//   norm_flush                      the workgroup's counters to memory
//
// Everything is __forceinline__: each kernel keeps its own launch bounds and its registers are its own.
#pragma once

#include "himut_device.h"

namespace himut {

struct NormArgs {
    Params P;
    SiteSets S;
    const GtLut* lut;
    Reads R;
    Chunks C;
    Phase H;
    const uint8_t* refseq;       // the contig as the FASTA holds it
    int64_t reflen;
    uint8_t cls[256];            // byte -> class id
    int K;                       // number of classes
    int cA, cC, cG, cT;          // class ids of the four bases
    uint8_t alt_order[12];       // [ref allele][0..2]: list(base_set.difference(ref)) as alleles
    int non_human;
    unsigned long long* ccs_tri; // [K^3]
    unsigned long long* ref_tri;
    unsigned long long* log;     // [14]
    int* err;
};

// ---------------------------------------------------------------------------------------
// A workgroup's counters: rows 1..13 of norm.log and the 32 trinucleotide bins of upper-case ACGT, added up in LDS and
// flushed once (norm_flush); the genotype priors beside them.
struct NormTally {
    double prior[4];
    unsigned int log[16];
    unsigned int ccs[32], ref[32];
};

__device__ __forceinline__ void norm_tally_init(NormTally& T, const NormArgs& A) {
    const int tid = threadIdx.x;
    if (tid < 4) T.prior[tid] = A.lut->prior[tid];
    if (tid < 16) T.log[tid] = 0;
    if (tid < 32) { T.ccs[tid] = 0; T.ref[tid] = 0; }
}

__device__ __forceinline__ void norm_flush(const NormTally& T, const NormArgs& A, int bad) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < 14 && T.log[tid]) atomicAdd(&A.log[tid], (unsigned long long)T.log[tid]);
    if (tid < 32 && (T.ccs[tid] || T.ref[tid])) {
        const int cl[4] = {A.cA, A.cC, A.cG, A.cT};
        const int64_t k = ((int64_t)cl[tid >> 3] * A.K + ((tid & 4) ? A.cT : A.cC)) * A.K + cl[tid & 3];
        atomicAdd(&A.ccs_tri[k], (unsigned long long)T.ccs[tid]);
        atomicAdd(&A.ref_tri[k], (unsigned long long)T.ref[tid]);
    }
    if (bad) atomicOr(A.err, bad);
}

// ---------------------------------------------------------------------------------------
// The state of one position.  cnt: bases of A, T, G, C, then insertions and deletions; S: the three tables' sums per
// allele.  The reference allele's count and sums are kept apart (nref; R0, R1, R2) and take their places in cnt and S in
// the classification.  The four small counters that every cell of a column may touch travel as 16-bit fields of two
// words (acc1: insertions | deletions << 16, acc2: reference bases | callable bases << 16) and are emptied (drain) into
// cnt[4], cnt[5], nref and tri_sum before a field can run over.
// (cnt is a vector type, which is what the compiler made of the bare array the kernels had before the struct: as six
//  separate counts the column walk comes out a tenth longer -- 359 instructions against 329 in k_callmap_sweep -- and the
//  map sweep measured 0.035 ms slower than before, 7.29 against 7.26 ms)
typedef uint32_t norm_u32x6 __attribute__((ext_vector_type(6)));
struct NormPos {
    norm_u32x6 cnt;
    GtSums S;
    double R0, R1, R2;
    uint32_t nref;
    uint32_t tri_sum, h0, h1;    // callable bases; bases of haplotype 0 and 1
    bool bq0;                    // a base of quality 0
    uint32_t acc1, acc2;

    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int k = 0; k < 6; k++) cnt[k] = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) { S[0][b] = 0.0; S[1][b] = 0.0; S[2][b] = 0.0; }
        R0 = 0.0; R1 = 0.0; R2 = 0.0;
        nref = 0;
        tri_sum = 0; h0 = 0; h1 = 0;
        bq0 = false;
        acc1 = 0; acc2 = 0;
    }

    __device__ __forceinline__ void drain() {
        cnt[4] += acc1 & 0xffffu; cnt[5] += acc1 >> 16; nref += acc2 & 0xffffu; tri_sum += acc2 >> 16;
        acc1 = 0; acc2 = 0;
    }

    // The tile sweep's update for cell v of the column.  (th, tt, te) are the table values of the cell's quality if the
    // cell is the reference allele and +0.0 otherwise (the caller reads entry 256, a zero row, for those), so the
    // reference allele's sums need no select.  lut: the three tables in LDS; hp: the row's haplotype, read in phased
    // runs only.
    __device__ __forceinline__ void cell(uint32_t v, bool use, bool isref, const uint32_t* hp, double th, double tt, double te,
                                         const double* lut, bool phase, int& bad) {
        const uint32_t c = v & 7u;
        const bool base = use && c < 4;
        const uint32_t q = v >> 8;
        bq0 = bq0 || (base && q == 0);
        R0 = R0 + th; R1 = R1 + tt; R2 = R2 + te;
        if (use && !isref && c <= CELL_OTHER) {             // rare: another allele, or a base outside ATGC
            if (c == CELL_OTHER) bad |= 1 << HIMUT_ERR_BASE;
            const double vh = lut[q], vt = lut[257 + q], ve = lut[514 + q];
#pragma unroll
            for (int b = 0; b < 4; b++) {
                if ((int)c == b) {
                    cnt[b]++;
                    S[0][b] = S[0][b] + vh;
                    S[1][b] = S[1][b] + vt;
                    S[2][b] = S[2][b] + ve;
                }
            }
        }
        uint32_t callable = base ? ((v >> 4) & 1u) : 0u;
        if (phase) {
            const uint32_t h = *hp;
            h0 += (base && h == HAP_0) ? 1u : 0u;
            h1 += (base && h == HAP_1) ? 1u : 0u;
            if (h != HAP_0 && h != HAP_1) callable = 0;
        }
        acc1 += (use ? ((v >> 3) & 1u) : 0u) | ((use && c == CELL_DEL) ? 0x10000u : 0u);
        acc2 += (isref ? 1u : 0u) | (callable << 16);
    }
};

// ---------------------------------------------------------------------------------------
// A position's verdict: its row of norm.log (2 unphased, 3 het, 4 hetalt, 5 homalt, 7 indel, 8 depth, 9 allele balance,
// 10 low GQ, 11 panel of normals, 12 common SNP, 13 callable), or where the reference's loop goes on to the next
// position without a row: no reference base, no callable base, a base of quality 0 (which fails the run).
enum : int { NORM_V_BQ0 = -1, NORM_V_NO_REF = 0, NORM_V_NO_BASE = 1, NORM_V_UNPHASED = 2 };

// get_germ_gq's gap: the ten PLs without allele `skip` (kept out of genotype(): the kernels take more registers when both
// forms go through it).  One position in thirty gets here.
__device__ __forceinline__ int norm_gq_without(const GtSums& S, const double* prior, int ref, int skip) {
    // (the priors are read from LDS again here, which this compiler-only barrier sees to: without it the ten values
    //  genotype() read are kept for this evaluation, across the counters and the site look-ups, and k_norm_tile spills
    //  them -- some 40 bytes of scratch a lane more, against the 36 the kernel had in all before; k_norm_dirty and
    //  k_callmap_sweep take 121 and 127 registers with the values kept, 109 and 111 without)
    asm volatile("" ::: "memory");
    double b2best = 0.0, b2second = 0.0;
#pragma unroll
    for (int g = 0; g < 10; g++) {
        const int b1 = (int)HIMUT_GT_B1(g), b2 = (int)HIMUT_GT_B2(g);
        double acc = 0.0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            if (b == skip) continue;
            double term;
            if (b1 == b2 && b == b1) term = S[0][b];
            else if (b1 != b2 && (b == b1 || b == b2)) term = S[1][b];
            else term = S[2][b];
            acc = acc + term;
        }
        acc = acc + prior[gt_state_of(b1, b2, ref)];
        const double pl = acc * -10.0;
        if (g == 0) b2best = pl;
        else if (pl < b2best) { b2second = b2best; b2best = pl; }
        else if (g == 1 || pl < b2second) b2second = pl;
    }
    const double g2 = b2second - b2best;
    return g2 < 99.0 ? (int)g2 : 99;
}

// The classification of position rpos (reference allele ref, -1: none) from its drained state.  Adds the position's
// callable bases to the counters that are no verdict's own (rows 1 and 2 of an unphased position, row 6 of a
// homozygous-reference one); the verdict's row is norm_tally's.
__device__ __forceinline__ int norm_classify(NormPos& p, const NormArgs& A, NormTally& T, int ref, int64_t rpos, bool phase, int& bad) {
    if (ref < 0) return NORM_V_NO_REF;
    if (p.tri_sum == 0) return NORM_V_NO_BASE;
#pragma unroll
    for (int b = 0; b < 4; b++) if (b == ref) { p.cnt[b] = p.nref; p.S[0][b] = p.R0; p.S[1][b] = p.R1; p.S[2][b] = p.R2; }
    if (phase && !((int64_t)p.h0 >= A.P.p.min_hap_count && (int64_t)p.h1 >= A.P.p.min_hap_count)) {
        atomicAdd(&T.log[1], p.tri_sum);
        atomicAdd(&T.log[2], p.tri_sum);
        return NORM_V_UNPHASED;
    }
    if (p.bq0) { bad |= 1 << HIMUT_ERR_BQ0; return NORM_V_BQ0; }
    const Genotype gt = genotype(p.S, T.prior, ref);
    const int gq = gt.gq;
    const int state = gt_state_of((int)HIMUT_GT_B1(gt.best), (int)HIMUT_GT_B2(gt.best), ref);
    const uint32_t depth = p.cnt[0] + p.cnt[1] + p.cnt[2] + p.cnt[3] + p.cnt[5];
    uint32_t ref_count = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) if (b == ref) ref_count = p.cnt[b];
    if (state == 1) return 3;
    if (state == 2) return 4;
    if (state == 3) return 5;
    atomicAdd(&T.log[6], p.tri_sum);
    if (p.cnt[5] != 0 || p.cnt[4] != 0) return 7;
    if ((int64_t)depth > A.P.p.md_threshold) return 8;
    if (depth == ref_count) {
        if (gq < A.P.p.min_gq) return 10;
        if ((int64_t)ref_count < A.P.p.min_ref_count) return 9;
        return 13;
    }
    uint32_t ac[3] = {0, 0, 0};
    const int32_t tpos = (int32_t)rpos + 1;
    const SiteSets& St = A.S;
    const bool site_maybe = !A.non_human && (int64_t)tpos < St.nposbits && ((St.posbits[tpos >> 5] >> (tpos & 31)) & 1u);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int aidx = A.alt_order[ref * 3 + a];
        uint32_t c = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) if (b == aidx) c = p.cnt[b];
        ac[a] = c;
        if (c == 0 || !site_maybe) continue;
        const uint64_t key = ((uint64_t)(uint32_t)tpos << 4) | ((uint64_t)ref << 2) | (uint64_t)aidx;
        if (key_in(St.pon, St.npon, key)) return 11;
        if (key_in(St.com, St.ncom, key)) return 12;
    }
    int bi = 0;                                             // the first of the largest counts
    uint32_t alt_count = ac[0];
    if (ac[1] > alt_count) { bi = 1; alt_count = ac[1]; }
    if (ac[2] > alt_count) { bi = 2; alt_count = ac[2]; }
    const int aidx = A.alt_order[ref * 3 + bi];
    const int gq2 = norm_gq_without(p.S, T.prior, ref, aidx);
    if (gq2 < A.P.p.min_gq) return 10;
    if (!((int64_t)ref_count >= A.P.p.min_ref_count && (int64_t)alt_count >= A.P.p.min_alt_count)) return 9;
    return 13;
}

// the trinucleotide bins of a callable position (row 13 of norm.log); refc: the reference's letter at rpos
__device__ __forceinline__ void norm_tribins(uint32_t tri_sum, const NormArgs& A, NormTally& T, int64_t rpos, int refc) {
    int t0 = 'N', t1 = 'N', t2 = 'N';
    if (rpos - 1 >= 0 && rpos + 2 <= A.reflen) {
        t0 = A.refseq[rpos - 1]; t1 = refc; t2 = A.refseq[rpos + 1];
        if (t1 == 'A' || t1 == 'G') {
            const int a0 = t2, a2 = t0;
            t0 = a0 == 'A' ? 'T' : a0 == 'T' ? 'A' : a0 == 'G' ? 'C' : a0 == 'C' ? 'G' : 'N';
            t1 = t1 == 'A' ? 'T' : 'C';
            t2 = a2 == 'A' ? 'T' : a2 == 'T' ? 'A' : a2 == 'G' ? 'C' : a2 == 'C' ? 'G' : 'N';
        }
    }
    auto acgt = [](int c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; };
    const int i0 = acgt(t0), i2 = acgt(t2);
    if (i0 >= 0 && i2 >= 0 && (t1 == 'C' || t1 == 'T')) {
        const int k = i0 * 8 + (t1 == 'T' ? 4 : 0) + i2;
        atomicAdd(&T.ccs[k], tri_sum);
        atomicAdd(&T.ref[k], 1u);
    } else {
        const int64_t k = ((int64_t)A.cls[t0] * A.K + A.cls[t1]) * A.K + A.cls[t2];
        atomicAdd(&A.ccs_tri[k], (unsigned long long)tri_sum);
        atomicAdd(&A.ref_tri[k], 1ULL);
    }
}

// the log counters and the trinucleotide bins of a classified position (verdict: what norm_classify returned)
__device__ __forceinline__ void norm_tally(int verdict, uint32_t tri_sum, const NormArgs& A, NormTally& T, int64_t rpos, int refc) {
    if (verdict < 3) return;
    atomicAdd(&T.log[1], tri_sum);
    atomicAdd(&T.log[verdict], tri_sum);
    if (verdict == 13) norm_tribins(tri_sum, A, T, rpos, refc);
}

// ---------------------------------------------------------------------------------------
// The tile sweep.  A workgroup of 256 threads takes tiles of 256 positions of one chunk; the reads that can cover a tile
// (the window index of its one or two 256-position blocks) are its rows.  Rows are handled NT_ROWS at a time: the four
// waves build the rows' cells in LDS -- a lane owns four consecutive positions of a row, finds them in the read's
// segment list, and loads the four qualities, the four packed bases and the four callable bits with one unaligned load
// each -- then every thread runs down its own column in read order.  Nothing is written to HBM.
//
// Which tile, when a kernel sweeps whole chunks (a row of the grid per chunk): workgroups are dealt round-robin over the
// eight XCDs (each with an L2 of its own), so the workgroups b, b + 8, b + 16 ... that run side by side on one XCD take
// NEIGHBOURING tiles of the chunk: a read's bytes at a tile boundary (its rows are 256 + 128 bytes at arbitrary offsets,
// i.e. partial 128-byte lines at both ends) are then asked for twice within microseconds and the second time come out
// of that L2.  gridDim.x is a multiple of 8.  (Speed only: any mapping gives the same counts.)
// A workgroup goes through several such tiles (its counters go to memory once): XCD class r = blockIdx.x & 7 owns the
// tiles [r * per, (r + 1) * per) of the chunk and its NT_Q workgroups take NT_Q neighbouring ones per step: workgroup
// blockIdx.x >> 3 of its class the tiles r * per + t for t = blockIdx.x >> 3, + gridDim.x >> 3, ... below per.
#ifndef HIMUT_NT_Q
#define HIMUT_NT_Q 16
#endif
#ifndef HIMUT_NT_NSG
#define HIMUT_NT_NSG 2
#endif
constexpr int NT_Q = HIMUT_NT_Q;         // workgroups per XCD class and chunk (each strides over its class's tiles)
constexpr int NT_ROWS = 48;
constexpr int NT_RPW = NT_ROWS / 4;    // rows per wave and batch

// per: by THIS chunk's length -- with the longest chunk's figure a short chunk would sit on the first XCDs only
__device__ __forceinline__ int64_t norm_tiles_per_class(const NormArgs& A, int chunk, int64_t tiles_per_class) {
    const int64_t span = (int64_t)A.C.end[chunk] - (int64_t)A.C.start[chunk];
    return min(tiles_per_class, ((span + 255) / 256 + 7) / 8);
}

struct NormLds {
    double lut[3 * 257];         // three tables of 256 qualities + a zero entry each (index 256)
    NormTally tally;
    __align__(16) uint16_t cells[NT_ROWS][256];
    int32_t tend[NT_ROWS];
    uint32_t hap[NT_ROWS];
};

__device__ __forceinline__ void norm_lds_init(NormLds& L, const NormArgs& A) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 3 * 256; i += 256) L.lut[(i >> 8) * 257 + (i & 255)] = A.lut->t[i >> 8][i & 255];
    if (tid < 3) L.lut[tid * 257 + 256] = 0.0;
    norm_tally_init(L.tally, A);
    __syncthreads();
}

// The tile of 256 positions from `base` of chunk `chunk` (base < the chunk's end), as a thread sees it: its own position
// and reference allele, and the tile's rows [lo, hi) of the reads.
struct NormTile {
    int64_t base, rpos, pairbase;
    int32_t cs, ce;              // the chunk
    int32_t lo, hi;
    int refc, ref;               // the reference's letter at rpos ('N' when !valid) and its allele (-1: none)
    bool valid;                  // rpos is a position of the chunk and of the reference string
};

__device__ __forceinline__ NormTile norm_tile_at(const NormArgs& A, int chunk, int64_t base, int32_t cs, int32_t ce, const int32_t* winlo,
                                                 const int32_t* winhi, int64_t nblk, bool phase, int& bad) {
    NormTile T;
    T.base = base; T.cs = cs; T.ce = ce;
    T.pairbase = phase ? A.C.pairoff[chunk] - A.C.rlo[chunk] : 0;
    T.rpos = base + (int)threadIdx.x;
    T.valid = T.rpos < ce;
    if (T.valid && (T.rpos < 0 || T.rpos >= A.reflen)) { bad |= 1 << HIMUT_ERR_ARG; T.valid = false; }   // IndexError in the reference
    T.refc = T.valid ? (int)A.refseq[T.rpos] : 'N';
    T.ref = char2allele(T.refc);
    // rows: the reads of the window index of the blocks under the tile
    const int64_t b0 = min(max(base, (int64_t)0) >> WIN_SHIFT, nblk - 1), b1 = min((base + 255) >> WIN_SHIFT, nblk - 1);
    T.lo = winlo[b0]; T.hi = winhi[b1];
    return T;
}

// The cells of rows [r0, r0 + nb) of the reads over tile T, into L.cells; the rows' ends and haplotypes beside them.
__device__ __forceinline__ void norm_build_rows(NormLds& L, const NormArgs& A, const Derived& D, const uint32_t* callable, const NormTile& T,
                                                int32_t r0, int nb, bool phase) {
    const int tid = threadIdx.x, lane = tid & 63, wv = uni(tid >> 6);
    const Reads& R = A.R;
    const int64_t base = T.base;
    const int32_t P0 = (int32_t)base + 4 * lane;              // this lane's four positions of every row
    // ---- the wave's rows, one per lane for the part that is a chain of dependent loads: read header, first
    //      segment that reaches the tile (binary search), the segments from there on
    const int myrow = wv + 4 * lane;                          // rows wv, wv + 4, ... of the batch
    const bool rowlane = lane < NT_RPW && myrow < nb;
    ReadMeta M;
    M.tstart = 0; M.tend = 0; M.nseg = 0; M.flags = RF_SECONDARY; M.segbase = 0; M.qoff = 0;
    if (rowlane) M = D.meta[r0 + myrow];
    const bool live_row = rowlane && !(M.flags & RF_SECONDARY) && M.nseg > 0 && M.tstart < base + 256 && M.tend >= base;
    int j0 = 0;
    if (live_row) {                                           // last segment that starts at or before the tile
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
        L.tend[myrow] = M.tend;
        uint32_t hp = HAP_NONE;
        if (phase && live_row && M.tstart < T.ce && M.tend > T.cs) hp = A.H.hap[T.pairbase + r0 + myrow];   // fetched by the chunk
        L.hap[myrow] = hp;
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
        *reinterpret_cast<uint2*>(&L.cells[row][4 * lane]) = packed;
    }
}

// Every thread down its column of the nb rows in L.cells, in read order.
__device__ __forceinline__ void norm_walk_columns(const NormLds& L, const NormTile& T, NormPos& p, int nb, bool phase, int& bad) {
    const int tid = threadIdx.x;
    // (what the loop reads of the tile, as plain locals: read through T the loop came out a quarter longer)
    const int ref = T.ref;
    const int32_t cs_ = T.cs;
    const bool edge = T.rpos <= T.cs;
    const bool any_edge = T.base <= T.cs;                     // only the chunk's first tile has such positions
    // NB rows at a time: the cells, then the three table values of each (the zero row unless the cell is the
    // reference allele), are loaded before any of them is used: the LDS latency is paid once per NB cells
    constexpr int NB = 2;      // (four at a time costs more in spills than the extra LDS round trips save)
    for (int i0 = 0; i0 < nb; i0 += NB) {
        uint32_t v4[NB];
        double th[NB], tt[NB], te[NB];
        bool use4[NB], ref4[NB];
#pragma unroll
        for (int k = 0; k < NB; k++) v4[k] = i0 + k < nb ? (uint32_t)L.cells[i0 + k][tid] : (uint32_t)CELL_EMPTY;
#pragma unroll
        for (int k = 0; k < NB; k++) {
            const uint32_t v = v4[k];
            const int ri = min(i0 + k, nb - 1);
            // an EMPTY cell, or a read this chunk did not fetch (normcounts.py:289), adds nothing
            use4[k] = (v & 15u) != CELL_EMPTY && !(any_edge && edge && !(L.tend[ri] > cs_));
            ref4[k] = use4[k] && (int)(v & 7u) == ref;
            const uint32_t qe = ref4[k] ? (v >> 8) : 256u;      // the zero row for everything but the reference allele
            th[k] = L.lut[qe]; tt[k] = L.lut[257 + qe]; te[k] = L.lut[514 + qe];
        }
#pragma unroll
        for (int k = 0; k < NB; k++)
            p.cell(v4[k], use4[k], ref4[k], &L.hap[min(i0 + k, nb - 1)], th[k], tt[k], te[k], L.lut, phase, bad);
    }
}

// Tile T's rows, NT_ROWS at a time, into the state of the thread's position (cleared here, drained at the end).  Every
// thread of the workgroup takes part, with a position of its own (T.valid) or without.
__device__ __forceinline__ void norm_sweep_tile(NormLds& L, const NormArgs& A, const Derived& D, const uint32_t* callable, const NormTile& T,
                                                NormPos& p, bool phase, int& bad) {
    p.clear();
    for (int32_t r0 = T.lo; r0 < T.hi; r0 += NT_ROWS) {
        const int nb = min(NT_ROWS, T.hi - r0);
        norm_build_rows(L, A, D, callable, T, r0, nb, phase);
        __syncthreads();
        if (T.valid) norm_walk_columns(L, T, p, nb, phase, bad);
        __syncthreads();
        if (((r0 - T.lo) / NT_ROWS & 511) == 511) p.drain();   // a pile tens of thousands of reads deep: empty the 16-bit fields
    }
    p.drain();
}

}  // namespace himut
