// The column back end that the call, germline, dbs and sites runs share: where a position's column lies in the column
// store, the walk over its slots that fills the pile, the genotype of the pile, the germline rule and the call run's
// non-phased verdict cascade.  __device__ functions and small structs only; each kernel lives with its run
// (himut_call.h, himut_germ.h, himut_dbs.h, himut_sites.h) and brings what is its own: a hook for the walk and its
// record layout.  Where the records go is the record back end's (himut_emit.h).
#pragma once

#include "himut_device.h"

namespace himut {

// a column of the store (its layout, BlockTab and PosIndex: himut_device.h): the slot of read lo + i is col[i * stride]
struct Column {
    const uint16_t* col;
    uint32_t n, stride;
    int32_t lo;
    bool ok;                     // inside the store's capacity
};

// the column of the marked position rpos, whose rank among the marked positions is u
__device__ __forceinline__ Column column_at(const PosIndex& X, const uint16_t* colstore, int64_t nslots, int32_t rpos, uint32_t u) {
    const BlockTab bt = X.bt[rpos >> 8];
    Column c;
    c.n = bt.ncnt & BT_N_MASK; c.stride = bt.ncnt >> 22; c.lo = bt.lo;
    const int64_t first = (int64_t)bt.boff + (int64_t)(u - bt.ufirst);
    // a column past the capacity (the store was sized before the slot count was known, or is kept from an earlier run):
    // the host runs again with exact sizes
    c.ok = !(c.n && first + (int64_t)(c.n - 1) * (int64_t)c.stride >= nslots);
    c.col = colstore + first;
    return c;
}

// the column of any position: an unmarked one, or one behind the bitmap, has no slots (n = 0)
__device__ __forceinline__ Column column_find(const PosIndex& X, const uint16_t* colstore, int64_t nslots, int32_t rpos) {
    if (rpos < 0 || (int64_t)(rpos >> 5) >= X.nwords || !((X.bits[rpos >> 5] >> (rpos & 31)) & 1u)) return {colstore, 0u, 0u, 0, true};
    return column_at(X, colstore, nslots, rpos, pos_rank(X, rpos));
}

// start <= tpos <= end for some region: the starts ascending, and the running maximum of their ends
__device__ __forceinline__ bool in_region(const int32_t* s_start, const int32_t* s_pmaxend, int64_t n, int32_t tpos) {
    const int64_t k = upper_bound(s_start, (int64_t)0, n, tpos);
    return k > 0 && s_pmaxend[k - 1] >= tpos;
}

// ---------------------------------------------------------------------------------------
// The pile of a column: allele counts and BQ sums (caller.py:44-72, bamlib.py:181-219) and the ordered likelihood sums
// of gtlib.py:72-96.  A kernel pays registers only for the members it reads (bqs, ref_bq, alt_bq, alt_hi fold away).
struct Pile {
    uint32_t cnt[6];             // A T G C, insertions, deletions
    uint32_t bqs[4];
    GtSums S;
    uint32_t ref_count, alt_count;
    uint32_t ref_bq, alt_bq;     // the two alleles' quality sums (= bqs[ref], bqs[alt])
    uint32_t alt_hi;             // alt reads with bq >= min_bq (caller.py:160-171)
    __device__ __forceinline__ uint32_t bases() const { return cnt[0] + cnt[1] + cnt[2] + cnt[3]; }
    __device__ __forceinline__ uint32_t depth() const { return bases() + cnt[5]; }    // bamlib.py:213-219
};

// A walk without a rule of its own.  A kernel's hook has these two members, inlined:
//   keep(i, v)        asked before slot i (cell word v, not empty) is counted: false leaves the read out of the pile
//   base(i, cell, q)  called after the base cell of slot i (allele `cell`, quality q) is summed
struct NoHook {
    __device__ __forceinline__ bool keep(uint32_t, uint32_t) { return true; }
    __device__ __forceinline__ void base(uint32_t, uint32_t, uint32_t) {}
};

// The slots of column C in fetch order into pile P, EB loads in flight.  The three fp64 sums of an allele are added
// from 0.0 in fetch order (gtlib.py:84-93).  Nearly every cell is the reference or the alt allele: those two have
// accumulators in locals of their own, put back afterwards (ref != alt; nothing else touches those entries); the
// four-way update runs for the rest.  alt = -1: no alt allele, its branch folds away.  bad: HIMUT_ERR_* bits.
template <int EB, class Hook>
__device__ __forceinline__ void walk_column(const Column& C, const double* s_lut, const int ref, const int alt, const int min_bq,
                                            Hook& hook, Pile& P, int& bad) {
#pragma unroll
    for (int b = 0; b < 6; b++) P.cnt[b] = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) { P.bqs[b] = 0; P.S[0][b] = 0.0; P.S[1][b] = 0.0; P.S[2][b] = 0.0; }
    uint32_t ref_count = 0, alt_count = 0, alt_hi = 0, Rq = 0, Aq = 0;
    double R0 = 0.0, R1 = 0.0, R2 = 0.0, A0 = 0.0, A1 = 0.0, A2 = 0.0;
    const uint32_t n = C.n, stride = C.stride;
    for (uint32_t i0 = 0; i0 < n; i0 += EB) {    // EB slots in flight: their addresses do not depend on each other
        uint32_t vv[EB];
#pragma unroll
        for (int k = 0; k < EB; k++) vv[k] = (i0 + k < n) ? (uint32_t)C.col[(int64_t)(i0 + k) * stride] : (uint32_t)CELL_EMPTY;
#pragma unroll
        for (int k = 0; k < EB; k++) {
            const uint32_t i = i0 + k;
            const uint32_t v = vv[k];
            const uint32_t cell = v & 7u;
            if ((v & 15u) == CELL_EMPTY) continue;
            if (!hook.keep(i, v)) continue;
            if (v & CELL_INS) P.cnt[4]++;
            if (cell < 4) {
                const uint32_t q = v >> 8;
                if (q == 0) bad |= 1 << HIMUT_ERR_BQ0;                     // gtlib.py:64
                const double vh = s_lut[q], vt = s_lut[256 + q], ve = s_lut[512 + q];
                if ((int)cell == ref) {
                    ref_count++; Rq += q;
                    R0 = R0 + vh; R1 = R1 + vt; R2 = R2 + ve;
                } else if ((int)cell == alt) {
                    alt_count++; Aq += q; if ((int)q >= min_bq) alt_hi++;
                    A0 = A0 + vh; A1 = A1 + vt; A2 = A2 + ve;
                } else {
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        if ((int)cell == b) {
                            P.cnt[b]++; P.bqs[b] += q;
                            P.S[0][b] = P.S[0][b] + vh;
                            P.S[1][b] = P.S[1][b] + vt;
                            P.S[2][b] = P.S[2][b] + ve;
                        }
                    }
                }
                hook.base(i, cell, q);
            } else if (cell == CELL_DEL) P.cnt[5]++;
            else if (cell == CELL_OTHER) bad |= 1 << HIMUT_ERR_BASE;       // caller.py:57
        }
    }
#pragma unroll
    for (int b = 0; b < 4; b++) {
        if (b == ref) { P.cnt[b] = ref_count; P.bqs[b] = Rq; P.S[0][b] = R0; P.S[1][b] = R1; P.S[2][b] = R2; }
        if (b == alt) { P.cnt[b] = alt_count; P.bqs[b] = Aq; P.S[0][b] = A0; P.S[1][b] = A1; P.S[2][b] = A2; }
    }
    P.ref_count = ref_count; P.alt_count = alt_count; P.ref_bq = Rq; P.alt_bq = Aq; P.alt_hi = alt_hi;
}

// the genotype LUT and the priors into LDS; the caller's __syncthreads() follows
__device__ __forceinline__ void stage_gt_lut(const GtLut* lut, double* s_lut, double* s_prior, int tid) {
    for (int i = tid; i < 3 * 256; i += 256) s_lut[i] = lut->t[i >> 8][i & 255];
    if (tid < 4) s_prior[tid] = lut->prior[tid];
}

struct Genotyped {
    int best, gq;                // genotype() of the pile
    int state;                   // 0 homref, 1 het, 2 hetalt, 3 homalt
    int g0, g1;                  // the two alleles as the reference prints them: a het's reference base first
};
__device__ __forceinline__ Genotyped genotype_column(const Pile& P, const double* s_prior, int ref) {
    const Genotype gt = genotype(P.S, s_prior, ref);
    Genotyped g;
    g.best = gt.best; g.gq = gt.gq;
    g.g0 = (int)HIMUT_GT_B1(gt.best); g.g1 = (int)HIMUT_GT_B2(gt.best);
    g.state = gt_state_of(g.g0, g.g1, ref);
    if (g.g0 != ref && ((g.g0 == ref) + (g.g1 == ref)) == 1) { const int tmp = g.g0; g.g0 = g.g1; g.g1 = tmp; }  // gtlib.py:133-134
    return g;
}

// the genotype explains (ref, alt) as germline (caller.py:111-147)
__device__ __forceinline__ bool is_germ_gt(const Genotyped& g, const Pile& P, int ref, int alt) {
    if (g.state == 1) return g.g0 == ref && g.g1 == alt;
    if (g.state == 2) {
        uint32_t c0 = 0, c1 = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) { if (g.g0 == b) c0 = P.cnt[b]; if (g.g1 == b) c1 = P.cnt[b]; }
        return P.bases() == c0 + c1 && (alt == g.g0 || alt == g.g1);
    }
    if (g.state == 3) return P.ref_count == 0 && (g.g0 == alt && g.g1 == alt);
    return alt == g.g0;
}

// The call run's non-phased cascade (caller.py:332-550) on a column that is_germ_gt did not drop: a HIMUT_ST_* value.
// LowGQ and LowBQ come ahead of the site sets: most candidates end there, without the look-up.
__device__ __forceinline__ int call_verdict(const Params& P, const SiteSets& St, const Genotyped& g, const Pile& pile, int32_t tpos, int ref,
                                            int alt) {
    if (g.state == 1) return HIMUT_ST_HET;
    if (g.state == 2) return HIMUT_ST_HETALT;
    if (g.state == 3) return HIMUT_ST_HOMALT;
    if (pile.cnt[5] != 0 || pile.cnt[4] != 0) return HIMUT_ST_INDEL;
    if (g.gq < P.p.min_gq) return HIMUT_ST_LOWGQ;
    if (pile.alt_hi == 0) return HIMUT_ST_LOWBQ;
    const uint64_t key = ((uint64_t)(uint32_t)tpos << 4) | ((uint64_t)ref << 2) | (uint64_t)alt;
    const bool site_maybe = (int64_t)tpos < St.nposbits && ((St.posbits[tpos >> 5] >> (tpos & 31)) & 1u);
    if (site_maybe && key_in(St.pon, St.npon, key)) return HIMUT_ST_PON;
    if (site_maybe && key_in(St.com, St.ncom, key)) return HIMUT_ST_COMSNP;
    if (!((int64_t)pile.ref_count >= P.p.min_ref_count && (int64_t)pile.alt_count >= P.p.min_alt_count)) return HIMUT_ST_LOWDEPTH;
    if ((int64_t)pile.depth() > P.p.md_threshold) return HIMUT_ST_HIGHDEPTH;
    return HIMUT_ST_PASS;
}

// place of a verdict in the cascade's order: HetSite .. ComSnp 0 .. 7, LowDepth 8, HighDepth 9, anything else (PASS) 10
__device__ __forceinline__ int verdict_rank(int st) {
    return st == HIMUT_ST_HET ? 0 : st == HIMUT_ST_HETALT ? 1 : st == HIMUT_ST_HOMALT ? 2 : st == HIMUT_ST_INDEL ? 3 :
           st == HIMUT_ST_LOWGQ ? 4 : st == HIMUT_ST_LOWBQ ? 5 : st == HIMUT_ST_PON ? 6 : st == HIMUT_ST_COMSNP ? 7 :
           st == HIMUT_ST_LOWDEPTH ? 8 : st == HIMUT_ST_HIGHDEPTH ? 9 : 10;
}

}  // namespace himut
