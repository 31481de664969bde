// Device code of the germline run (himut_run_germline): the columns the call run throws away as germline, kept.
//
// The run shares the call run's front half -- k_parse_cs marks the substitution positions of every pile read in the
// bitmap, k_block_sums / k_block_table3 index the marked positions, k_stream_capture fills the column store (no
// proposals: its mask is null) -- and adds three kernels of its own:
//
//   k_germ_refbase    sixteen lanes per read: every substitution of a pile read names the reference base of its
//                     position, one-hot per marked rank (two reads that disagree leave two bits: HIMUT_ERR_CS); the
//                     substitutions whose cs reference base is n set a bitmap of their own (num_nref)
//   k_germline_eval   one workgroup per 8192 positions (32 blocks of the column index): the marked positions of its
//                     bitmap words are listed in LDS in position order, then one THREAD per marked position takes the
//                     column through the shared walk and genotype (himut_column.h) with the pile's mapq rule, runs
//                     the run's own FILTER cascade and writes the record (pack_record) at the workgroup's first rank +
//                     its place among the workgroup's records (wg_rank, once per round of 256 positions): position order
//   GermRuns          what the run gives the shared compaction (k_compact_runs, himut_emit.h): a workgroup's records
//                     start at its first rank; in the same launch the twelve counters are summed from the
//                     per-workgroup partial rows and the run's totals are left for the host
#pragma once

#include "himut_emit.h"

namespace himut {

struct GermArgs {
    himut_germline_params p;
    const GtLut* lut;
    Reads R;
    Derived D;
    PosIndex X;
    const int32_t* s_start;      // region starts ascending, and the running maximum of their ends
    const int32_t* s_pmaxend;
    int64_t nregion;
    const uint16_t* colstore;
    int64_t nslots;              // capacity of colstore
    uint32_t* refmask;           // per marked rank one byte: bit a = some pile read names allele a as the reference base
    const uint32_t* nrefbits;    // positions at which a pile read's substitution names n as the reference base
    int64_t cap_marked;          // capacity of refmask / recs (ranks)
    himut_record* recs;          // workgroup w's records start at its first rank
    uint32_t* wgcnt;             // records per workgroup
    uint32_t* logpart;           // 12 counters per workgroup
    int* err;
};

constexpr int GERM_WG_WORDS = 256;                    // bitmap words (32 positions each) per workgroup
constexpr int GERM_WG_BLOCKS = GERM_WG_WORDS / 8;     // blocks of the column index per workgroup

// the read is in the piles of the run: not secondary, mapq >= min_mapq
__device__ __forceinline__ bool germ_pile_read(const Reads& R, const Derived& D, int64_t r, int min_mapq) {
    return !(D.rflag[r] & RF_SECONDARY) && (int)R.mapq[r] >= min_mapq;
}

__global__ void __launch_bounds__(256) k_germ_refbase(Reads R, Derived D, PosIndex X, int min_mapq, uint32_t* refmask, int64_t cap_marked,
                                                      uint32_t* nrefbits, const int* err) {
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int gl = threadIdx.x & 15;
    if (r >= R.n || *err) return;
    if (!germ_pile_read(R, D, r, min_mapq)) return;
    const ReadMeta M = D.meta[r];
    const int nm = D.nmis[r];
    const int32_t* mis = D.mis + M.segbase;
    const uint32_t* mq = D.mq + M.segbase;
    for (int e = gl; e < nm; e += 16) {
        const uint32_t v = mq[e];
        if (!(v & 16u)) continue;
        const int32_t rpos = mis[e] - 1;
        if (rpos < 0 || (int64_t)(rpos >> 5) >= X.nwords || !((X.bits[rpos >> 5] >> (rpos & 31)) & 1u)) continue;
        const uint32_t u = pos_rank(X, rpos);
        if ((int64_t)u >= cap_marked) continue;            // kept capacities too small: the host runs again
        atomicOr(refmask + (u >> 2), (1u << ((v >> 2) & 3u)) << (8 * (u & 3u)));
    }
    const int nn = D.nnsub[r];
    if (nn > 0) {
        const int64_t top = (R.cs_off[r + 1] >> 1) - (R.cs_off[r] >> 1);
        const Seg* segs = D.segs + M.segbase;
        for (int k = gl; k < nn; k += 16) {
            const int32_t q = (int32_t)(mq[top - k] >> 5);
            for (int j = 0; j < M.nseg; j++) {
                const Seg g = segs[j];
                if ((g.flags & SEG_DEL) || g.len <= 0 || q < g.q0 || q >= g.q0 + g.len) continue;
                const int32_t t = g.t0 + (q - g.q0);
                if (t >= 0 && (int64_t)(t >> 5) < X.nwords) atomicOr(nrefbits + (t >> 5), 1u << (t & 31));
                break;
            }
        }
    }
}

#ifndef HIMUT_GERM_WAVES
#define HIMUT_GERM_WAVES 4
#endif
#ifndef HIMUT_GERM_BATCH
#define HIMUT_GERM_BATCH 8
#endif
// The germline run's rules for the walk.  keep, under MAPQ (min_mapq > 0): the slot's read is looked up, its mapq decides
// whether it is in the pile.  base: which non-reference alleles have a read with bq >= min_bq.
template <bool MAPQ>
struct GermHook {
    const uint8_t* mapq;         // of the column's first read on
    const int min_mapq, min_bq, ref;
    uint32_t hi = 0;             // bit a: allele a has a read with bq >= min_bq
    __device__ __forceinline__ bool keep(uint32_t i, uint32_t) { return !(MAPQ && (int)mapq[i] < min_mapq); }
    __device__ __forceinline__ void base(uint32_t, uint32_t cell, uint32_t q) {
        if ((int)cell != ref && (int)q >= min_bq) hi |= 1u << cell;
    }
};

template <bool MAPQ>
__global__ void __launch_bounds__(256, HIMUT_GERM_WAVES) k_germline_eval(GermArgs A) {
    __shared__ double s_lut[3 * 256];
    __shared__ double s_prior[4];
    __shared__ uint16_t s_pos[GERM_WG_WORDS * 32];
    __shared__ int s_w[4];
    __shared__ uint32_t s_log[12];
    const int tid = threadIdx.x;
    stage_gt_lut(A.lut, s_lut, s_prior, tid);
    if (tid < 12) s_log[tid] = 0;
    const int64_t b0 = (int64_t)blockIdx.x * GERM_WG_BLOCKS;
    const int64_t wi = (int64_t)blockIdx.x * GERM_WG_WORDS + tid;
    const bool dead = *A.err != 0;
    // ---- this thread's bitmap word: its marked positions into the list, in position order
    uint32_t w = 0, nw = 0;
    if (!dead && wi < A.X.nwords) { w = A.X.bits[wi]; nw = A.nrefbits[wi]; }
    const WgRank listed = wg_rank_count<4>(__popc(w), s_w);
    int at = listed.rank, total = listed.total;
    for (uint32_t x = w; x; x &= x - 1) s_pos[at++] = (uint16_t)(tid * 32 + (__ffs((int)x) - 1));
    // positions at which only n is named as the reference base: counted, never evaluated
    uint32_t n_nref = 0;
    for (uint32_t x = nw & ~w; x; x &= x - 1)
        if (in_region(A.s_start, A.s_pmaxend, A.nregion, (int32_t)(wi * 32 + (__ffs((int)x) - 1)) + 1)) n_nref++;
    if (n_nref) atomicAdd(&s_log[1], n_nref);
    __syncthreads();
    const uint32_t u0 = total ? A.X.bt[b0].ufirst : 0u;
    const int32_t p_base = (int32_t)(b0 << 8);
    int nrec_wg = 0;             // records of the rounds so far (the same in every thread)
    int bad = 0;
    for (int i0 = 0; i0 < total; i0 += 256) {
        const int i = i0 + tid;
        bool emit = false;
        RecordWords rec;
        if (i < total) {
            const int32_t rpos = p_base + (int32_t)s_pos[i];
            const int32_t tpos = rpos + 1;
            const uint32_t u = u0 + (uint32_t)i;
            const Column C = column_at(A.X, A.colstore, A.nslots, rpos, u);
            // a rank or a column past the capacities kept from an earlier run: the host runs again with exact sizes
            const bool fits = (int64_t)u < A.cap_marked && C.ok;
            if (fits && in_region(A.s_start, A.s_pmaxend, A.nregion, tpos)) {
                const uint32_t rm = (A.refmask[u >> 2] >> (8 * (u & 3u))) & 15u;
                const bool isn = (A.nrefbits[rpos >> 5] >> (rpos & 31)) & 1u;
                if (isn) {
                    atomicAdd(&s_log[1], 1u);
                    if (rm) bad |= 1 << HIMUT_ERR_CS;               // n here, a base there
                } else if (rm & (rm - 1)) bad |= 1 << HIMUT_ERR_CS;  // two reads, two reference bases
                else if (rm) {
                    const int ref = __ffs((int)rm) - 1;
                    GermHook<MAPQ> hook{A.R.mapq + C.lo, A.p.min_mapq, A.p.min_bq, ref};
                    Pile pile;
                    walk_column<HIMUT_GERM_BATCH>(C, s_lut, ref, -1, 0, hook, pile, bad);      // no alt allele
                    const Genotyped g = genotype_column(pile, s_prior, ref);
                    const int state = g.state, g0 = g.g0, g1 = g.g1;
                    const uint32_t* cnt = pile.cnt;
                    const uint32_t hi = hook.hi;
                    atomicAdd(&s_log[0], 1u);
                    atomicAdd(&s_log[2 + state], 1u);
                    // the alt alleles: the genotype's alleles other than the reference base
                    const int a0 = state == 1 ? g1 : g0, a1 = state == 2 ? g1 : a0;
                    int status = HIMUT_ST_PASS;
                    if (state != 0) {
                        uint32_t c0 = 0, c1 = 0;
#pragma unroll
                        for (int b = 0; b < 4; b++) { if (a0 == b) c0 = cnt[b]; if (a1 == b) c1 = cnt[b]; }
                        if (g.gq < A.p.min_gq) status = HIMUT_ST_LOWGQ;
                        else if (!((hi >> a0) & 1u) || !((hi >> a1) & 1u)) status = HIMUT_ST_LOWBQ;
                        else if ((int64_t)c0 < A.p.min_alt_count || (int64_t)c1 < A.p.min_alt_count ||
                                 (state == 1 && (int64_t)pile.ref_count < A.p.min_ref_count)) status = HIMUT_ST_LOWDEPTH;
                        else if ((int64_t)pile.depth() > A.p.md_threshold) status = HIMUT_ST_HIGHDEPTH;
                        const int slot = status == HIMUT_ST_PASS ? 6 : status == HIMUT_ST_LOWGQ ? 7 : status == HIMUT_ST_LOWBQ ? 8 :
                                         status == HIMUT_ST_LOWDEPTH ? 9 : 10;
                        atomicAdd(&s_log[slot], 1u);
                    }
                    emit = state != 0 || A.p.report_homref != 0;
                    rec = pack_record(tpos, -1, -1, g.gq, ref, a0, g0, g1, status, state, 0u, cnt, pile.bqs);   // no chunk, no phase set
                }
            }
        }
        // ---- the round's records behind the earlier rounds', in list (= position) order
        const WgRank e = wg_rank<4>(emit, s_w);
        // nrec_wg + e.rank <= i: inside the workgroup's ranks, which fit the capacity (checked above)
        if (emit) rec.store(A.recs + ((int64_t)u0 + nrec_wg + e.rank));
        nrec_wg += e.total;
        __syncthreads();             // s_w is the next round's too
    }
    if (bad) atomicOr(A.err, bad);
    __syncthreads();
    if (tid == 0) A.wgcnt[blockIdx.x] = (uint32_t)nrec_wg;
    if (tid < 12) A.logpart[(int64_t)blockIdx.x * 12 + tid] = s_log[tid];
}

// The germline run's side of k_compact_runs: workgroup w's records start at its first rank.  Workgroup 0 also adds up the
// counters; the last one leaves the run's totals: marked positions, column-store slots (what the host compares with the
// capacities).
struct GermRuns {
    const himut_record* recs;
    const uint32_t *logpart, *blkoff, *blkslots;
    PosIndex X;
    int64_t cap_marked;
    unsigned long long *nmarked, *nslots, *log;
    __device__ __forceinline__ const himut_record* src(int64_t w, uint32_t& mine) const {
        const int64_t u0 = (int64_t)X.bt[w * GERM_WG_BLOCKS].ufirst;
        return u0 + (int64_t)mine <= cap_marked ? recs + u0 : nullptr;
    }
    __device__ __forceinline__ void tail() const {
        if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
            const FrontTotals t = front_totals_of(X, blkoff, blkslots);
            *nmarked = t.marked; *nslots = t.slots;
        }
        if (blockIdx.x == 0 && threadIdx.x < 12) {
            unsigned long long s = 0;
            for (int64_t k = 0; k < (int64_t)gridDim.x; k++) s += logpart[k * 12 + threadIdx.x];
            log[threadIdx.x] = s;
        }
    }
};

}  // namespace himut
