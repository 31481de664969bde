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
//                     the run's own FILTER cascade and writes the record at the workgroup's first rank + its place
//                     among the workgroup's records (a ballot): position order
//   k_germ_compact    every workgroup adds up the record counts in front of it and moves its run of records there;
//                     the twelve counters are summed from the per-workgroup partial rows
#pragma once

#include "himut_column.h"

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
    __shared__ int s_w[4], s_e[4];
    __shared__ uint32_t s_log[12];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    stage_gt_lut(A.lut, s_lut, s_prior, tid);
    if (tid < 12) s_log[tid] = 0;
    const int64_t b0 = (int64_t)blockIdx.x * GERM_WG_BLOCKS;
    const int64_t wi = (int64_t)blockIdx.x * GERM_WG_WORDS + tid;
    const bool dead = *A.err != 0;
    // ---- this thread's bitmap word: its marked positions into the list, in position order
    uint32_t w = 0, nw = 0;
    if (!dead && wi < A.X.nwords) { w = A.X.bits[wi]; nw = A.nrefbits[wi]; }
    const int c = __popc(w);
    const int incl = wave_incl_add(c, lane);
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    int at = incl - c;
    for (int k = 0; k < wv; k++) at += s_w[k];
    const int total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
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
        uint4 w0 = make_uint4(0, 0, 0, 0), w1 = w0, w2 = w0, w3 = w0;
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
                    w0.x = (uint32_t)tpos; w0.y = 0xffffffffu; w0.z = 0xffffffffu; w0.w = (uint32_t)g.gq;
                    w1.x = (uint32_t)allele2char(ref) | ((uint32_t)allele2char(a0) << 8) | ((uint32_t)allele2char(g0) << 16) |
                           ((uint32_t)allele2char(g1) << 24);
                    w1.y = (uint32_t)(status & 255) | ((uint32_t)state << 8);
                    w1.z = cnt[0]; w1.w = cnt[1];
                    w2.x = cnt[2]; w2.y = cnt[3]; w2.z = cnt[4]; w2.w = cnt[5];
                    w3.x = pile.bqs[0]; w3.y = pile.bqs[1]; w3.z = pile.bqs[2]; w3.w = pile.bqs[3];
                }
            }
        }
        // ---- the round's records behind the earlier rounds', in list (= position) order
        const unsigned long long eb = __ballot(emit);
        if (lane == 0) s_e[wv] = __popcll(eb);
        __syncthreads();
        int place = nrec_wg + (int)__popcll(eb & ((1ULL << lane) - 1ULL));
        for (int k = 0; k < wv; k++) place += s_e[k];
        if (emit) {      // place <= i: inside the workgroup's ranks, which fit the capacity (checked above)
            uint4* dst = reinterpret_cast<uint4*>(A.recs + ((int64_t)u0 + place));
            dst[0] = w0; dst[1] = w1; dst[2] = w2; dst[3] = w3;
        }
        nrec_wg += s_e[0] + s_e[1] + s_e[2] + s_e[3];
        __syncthreads();
    }
    if (bad) atomicOr(A.err, bad);
    __syncthreads();
    if (tid == 0) A.wgcnt[blockIdx.x] = (uint32_t)nrec_wg;
    if (tid < 12) A.logpart[(int64_t)blockIdx.x * 12 + tid] = s_log[tid];
}

// Workgroup w's records (wgcnt[w] of them, from its first rank on) to their place behind the records of the workgroups
// in front of it.  Workgroup 0 also adds up the counters; the last one leaves the run's totals: records, marked positions,
// column-store slots (what the host compares with the capacities).
__global__ void __launch_bounds__(256) k_germ_compact(const himut_record* recs, const uint32_t* wgcnt, const uint32_t* logpart, PosIndex X,
                                                      const uint32_t* blkoff, const uint32_t* blkslots, int64_t cap_marked, himut_record* out,
                                                      unsigned long long* nrec, unsigned long long* nmarked, unsigned long long* nslots,
                                                      unsigned long long* log) {
    __shared__ unsigned long long s_sum[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned long long part = 0;
    for (int64_t k = tid; k < (int64_t)blockIdx.x; k += 256) part += wgcnt[k];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d, 64);
    if (lane == 0) s_sum[wv] = part;
    __syncthreads();
    const unsigned long long base = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    const uint32_t mine = wgcnt[blockIdx.x];
    if (mine) {
        const int64_t u0 = (int64_t)X.bt[(int64_t)blockIdx.x * GERM_WG_BLOCKS].ufirst;
        if (u0 + (int64_t)mine <= cap_marked) {
            const uint4* src = reinterpret_cast<const uint4*>(recs + u0);
            uint4* dst = reinterpret_cast<uint4*>(out + base);
            for (int64_t k = tid; k < (int64_t)mine * 4; k += 256) dst[k] = src[k];
        }
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) {
        *nrec = base + mine;
        const BlockTab t = X.bt[X.nblk - 1];
        *nmarked = (unsigned long long)t.ufirst + (unsigned long long)(t.ncnt >> 22);
        *nslots = (unsigned long long)blkoff[X.nblk - 1] + (unsigned long long)blkslots[X.nblk - 1];
    }
    if (blockIdx.x == 0 && tid < 12) {
        unsigned long long s = 0;
        for (int64_t k = 0; k < (int64_t)gridDim.x; k++) s += logpart[k * 12 + tid];
        log[tid] = s;
    }
}

}  // namespace himut
