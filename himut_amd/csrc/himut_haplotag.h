// The kernel of himut_run_haplotag (himut_haplotag.hip): each read's haplotype from the contig's phased hetSNPs, and
// what the reads say about each hetSNP.  The contract is include/himut_hip.h (himut_run_haplotag) and DESIGN.md section 8,
// row 15.
//
//   k_haplotag   sixteen lanes per read: the read's row, the five allele tallies of every hetSNP it spans, behind the
//                read's verdict agree / disagree of the hetSNPs of its chosen set it voted at, the counters
//
// The lanes find the read's hetSNPs by a search of the sorted positions and then take a hetSNP each, in turns of sixteen:
// the base by a search of the read's segments (k_read_hap's, himut_reads.h).  agree and disagree depend on nothing but
// the read's own verdict, so nothing is handed from one workgroup to another.
#pragma once

#include "himut_device.h"

namespace himut {

static_assert(sizeof(himut_haplotag_row) == 32, "himut_haplotag_row is 32 bytes (HAPLOTAG_ROW_DTYPE of _ffi.py)");
static_assert(offsetof(himut_haplotag_row, set) == 4 && offsetof(himut_haplotag_row, n0) == 8 &&
              offsetof(himut_haplotag_row, n_other) == 16 && offsetof(himut_haplotag_row, n_lowbq) == 24 &&
              offsetof(himut_haplotag_row, n_sets) == 28 && offsetof(himut_haplotag_row, hap) == 30 &&
              offsetof(himut_haplotag_row, status) == 31, "himut_haplotag_row layout");
static_assert(sizeof(himut_haplotag_snp) == 32, "himut_haplotag_snp is 32 bytes (HAPLOTAG_SNP_DTYPE of _ffi.py)");
static_assert(offsetof(himut_haplotag_snp, n_ref) == 0 && offsetof(himut_haplotag_snp, n_alt) == 4 &&
              offsetof(himut_haplotag_snp, n_other) == 8 && offsetof(himut_haplotag_snp, n_del) == 12 &&
              offsetof(himut_haplotag_snp, n_lowbq) == 16 && offsetof(himut_haplotag_snp, agree) == 20 &&
              offsetof(himut_haplotag_snp, disagree) == 24, "himut_haplotag_snp layout: the kernel indexes its words");

// what a read shows at a hetSNP; the first five are the word of the hetSNP's row that counts it
enum : int { HT_REF = 0, HT_ALT = 1, HT_OTHER = 2, HT_DEL = 3, HT_LOWBQ = 4, HT_UNCOVERED = 5, HT_AGREE = 5, HT_DISAGREE = 6 };
// the counters, in the order of himut_get_haplotag's log
enum : int { HL_READS = 0, HL_PILE, HL_HAP0, HL_HAP1, HL_NOSNP, HL_NOVOTE, HL_LOWSUPPORT, HL_CONFLICT, HL_MULTISET, HL_VOTES,
             HL_OTHER, HL_DEL, HL_LOWBQ, HL_COUNT };

struct HaplotagArgs {
    Reads R;
    Derived D;
    const int32_t* pos1;      // the hetSNPs: 1-based, strictly ascending
    const uint8_t *ref, *alt; // ASCII
    const uint8_t* bit;       // the allele on the first haplotype
    const int32_t* set;
    int64_t nsnps;
    int32_t min_mapq, min_bq, min_snps, min_agree_permille;
    himut_haplotag_row* rows; // one per read
    uint32_t* snps;           // eight words per hetSNP (himut_haplotag_snp)
    unsigned long long* log;  // HL_COUNT counters
    int* err;
};

// over the sixteen lanes of a read (one row of the wave); every lane takes part and gets the result
__device__ __forceinline__ uint32_t group16_sum(uint32_t v) {
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 16);
    return v;
}
__device__ __forceinline__ int32_t group16_min(int32_t v) {
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, 16));
    return v;
}

// The hetSNPs a read spans, tstart <= pos1 - 1 < tend, as [*idx, *jdx): the first position > tstart and the first > tend.
// (Every lane searches for itself: a search the sixteen lanes share, seventeen ways a round, measured 2.5 % of the run and
// was taken out again -- DESIGN.md, row 15.)
__device__ __forceinline__ void haplotag_span(const int32_t* pos1, int64_t n, int32_t tstart, int32_t tend, int64_t* idx, int64_t* jdx) {
    *idx = upper_bound(pos1, (int64_t)0, n, tstart);
    *jdx = upper_bound(pos1, *idx, n, tend);
}

// a read's segments and bases, for the look-ups of one lane
struct HaplotagRead {
    const Seg* segs;
    int ns;
    int64_t qo;
};

// what the read shows at hetSNP g (HT_*): the first segment that ends behind the position (segments are in order and do
// not overlap), then deletion, quality, base -- in this order
__device__ __forceinline__ int haplotag_look(const HaplotagArgs& A, const HaplotagRead& X, int64_t g) {
    const int32_t rpos = A.pos1[g] - 1;
    int lo = 0, hi = X.ns;
    while (lo < hi) { const int m = (lo + hi) >> 1; if (rpos >= X.segs[m].t0 + X.segs[m].len) lo = m + 1; else hi = m; }
    if (lo >= X.ns) return HT_UNCOVERED;
    const Seg sg = X.segs[lo];
    if (rpos < sg.t0) return HT_UNCOVERED;
    if (sg.flags & SEG_DEL) return HT_DEL;
    const int64_t q = X.qo + sg.q0 + (rpos - sg.t0);
    if ((int32_t)A.R.bq[q] < A.min_bq) return HT_LOWBQ;
    const int qb = nib2char(nib_at(A.R.seq, q));
    return qb == (int)A.ref[g] ? HT_REF : (qb == (int)A.alt[g] ? HT_ALT : HT_OTHER);
}

__global__ void __launch_bounds__(256) k_haplotag(HaplotagArgs A) {
    __shared__ unsigned int s_log[HL_COUNT];
    if (threadIdx.x < HL_COUNT) s_log[threadIdx.x] = 0;
    __syncthreads();
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int gl = threadIdx.x & 15;
    if (r < A.R.n && *A.err == 0) {              // (a decode that failed left segments nobody should follow)
        himut_haplotag_row row;
        row.read = (int32_t)r; row.set = -1;
        row.n0 = row.n1 = row.n_other = row.n_del = row.n_lowbq = 0;
        row.n_sets = 0; row.hap = HAP_NONE; row.status = HIMUT_HT_NOTINPILE;
        const ReadMeta M = A.D.meta[r];
        const bool pile = !(M.flags & RF_SECONDARY) && (int32_t)A.R.mapq[r] >= A.min_mapq;
        uint32_t tv = 0, to = 0, td = 0, tl = 0;             // over every spanned hetSNP: votes, other, del, lowbq
        if (pile) {
            int64_t idx, jdx;
            haplotag_span(A.pos1, A.nsnps, M.tstart, M.tend, &idx, &jdx);
            const int64_t k = jdx - idx;
            if (k <= 0) row.status = HIMUT_HT_NOSNP;
            else {
                const HaplotagRead X = {A.D.segs + M.segbase, M.nseg, M.qoff};
                // the first turn's answers stay in registers: most reads span no more than sixteen hetSNPs
                int look0 = HT_UNCOVERED, h0 = 0;
                int32_t set0 = 0;
                int32_t nxt = INT32_MAX;                     // the smallest set with a vote
                uint32_t unc = 0;
                for (int64_t a0 = 0; a0 < k; a0 += 16) {
                    const int64_t g = idx + a0 + gl;
                    if (g >= jdx) continue;
                    const int look = haplotag_look(A, X, g);
                    const int32_t s = A.set[g];
                    if (a0 == 0) { look0 = look; set0 = s; h0 = look ^ (int)A.bit[g]; }
                    if (look == HT_UNCOVERED) { unc = 1; continue; }
                    atomicAdd(A.snps + 8 * g + look, 1u);
                    if (look <= HT_ALT) { tv++; nxt = min(nxt, s); }
                    else if (look == HT_OTHER) to++;
                    else if (look == HT_DEL) td++;
                    else tl++;
                }
                tv = group16_sum(tv); to = group16_sum(to); td = group16_sum(td); tl = group16_sum(tl);
                unc = group16_sum(unc);
                nxt = group16_min(nxt);
                if (unc && gl == 0) set_err(A.err, HIMUT_ERR_COVER);
                // the sets with a vote, from the smallest up: the one with the most votes, the lower index on a tie
                uint32_t b0 = 0, b1 = 0, bo = to, bd = td, bl = tl, nsets = 0;
                int32_t best = -1;
                for (int32_t cur = nxt; cur != INT32_MAX; cur = nxt) {
                    uint32_t c0 = 0, c1 = 0, co = 0, cd = 0, cl = 0;
                    nxt = INT32_MAX;
                    for (int64_t a0 = 0; a0 < k; a0 += 16) {
                        const int64_t g = idx + a0 + gl;
                        if (g >= jdx) continue;
                        const int32_t s = a0 == 0 ? set0 : A.set[g];
                        if (s < cur) continue;
                        const int look = a0 == 0 ? look0 : haplotag_look(A, X, g);
                        if (s > cur) { if (look <= HT_ALT) nxt = min(nxt, s); continue; }
                        if (look <= HT_ALT) { if ((a0 == 0 ? h0 : (look ^ (int)A.bit[g])) == 0) c0++; else c1++; }
                        else if (look == HT_OTHER) co++;
                        else if (look == HT_DEL) cd++;
                        else if (look == HT_LOWBQ) cl++;
                    }
                    c0 = group16_sum(c0); c1 = group16_sum(c1); co = group16_sum(co); cd = group16_sum(cd); cl = group16_sum(cl);
                    nxt = group16_min(nxt);
                    nsets++;
                    if (best < 0 || c0 + c1 > b0 + b1) { best = cur; b0 = c0; b1 = c1; bo = co; bd = cd; bl = cl; }
                }
                row.set = best; row.n0 = b0; row.n1 = b1; row.n_other = bo; row.n_del = bd; row.n_lowbq = bl;
                row.n_sets = (uint16_t)min(nsets, 65535u);
                const unsigned long long votes = (unsigned long long)b0 + b1, top = max(b0, b1);
                if (best < 0) row.status = HIMUT_HT_NOVOTE;
                else if (votes < (unsigned long long)A.min_snps) row.status = HIMUT_HT_LOWSUPPORT;
                else if (b0 == b1 || top * 1000ULL < (unsigned long long)A.min_agree_permille * votes) row.status = HIMUT_HT_CONFLICT;
                else { row.status = HIMUT_HT_ASSIGNED; row.hap = b0 > b1 ? HAP_0 : HAP_1; }
                // an Assigned read's votes at the hetSNPs of its chosen set: with its haplotype, or against it
                if (row.status == HIMUT_HT_ASSIGNED) {
                    for (int64_t a0 = 0; a0 < k; a0 += 16) {
                        const int64_t g = idx + a0 + gl;
                        if (g >= jdx) continue;
                        if ((a0 == 0 ? set0 : A.set[g]) != best) continue;
                        const int look = a0 == 0 ? look0 : haplotag_look(A, X, g);
                        if (look > HT_ALT) continue;
                        const int h = a0 == 0 ? h0 : (look ^ (int)A.bit[g]);
                        atomicAdd(A.snps + 8 * g + (h == (int)row.hap ? HT_AGREE : HT_DISAGREE), 1u);
                    }
                }
            }
        }
        if (gl == 0) {
            A.rows[r] = row;
            atomicAdd(&s_log[HL_READS], 1u);
            if (pile) {
                atomicAdd(&s_log[HL_PILE], 1u);
                if (row.status == HIMUT_HT_ASSIGNED) atomicAdd(&s_log[row.hap == HAP_0 ? HL_HAP0 : HL_HAP1], 1u);
                else atomicAdd(&s_log[HL_NOSNP + (row.status - HIMUT_HT_NOSNP)], 1u);
                if (row.n_sets >= 2) atomicAdd(&s_log[HL_MULTISET], 1u);
                if (tv) atomicAdd(&s_log[HL_VOTES], tv);
                if (to) atomicAdd(&s_log[HL_OTHER], to);
                if (td) atomicAdd(&s_log[HL_DEL], td);
                if (tl) atomicAdd(&s_log[HL_LOWBQ], tl);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < HL_COUNT && s_log[threadIdx.x]) atomicAdd(A.log + threadIdx.x, (unsigned long long)s_log[threadIdx.x]);
}

}  // namespace himut
