// Device code of the sites run (himut_run_sites): the substitutions of a host-supplied site list genotyped on the call
// path's pile of another sample.  The contract is include/himut_hip.h (himut_run_sites) and DESIGN.md section 8, row 11.
//
// The run goes over the column front with the bitmap filled from the sites instead of from the reads: k_parse_cs runs
// under a parameter block whose query-length limits are closed, so no read passes the bitmap gate and the decode marks
// nothing (it still leaves the segment lists, the mismatch lists and the flags as always); k_sites_mark sets the sites'
// bits; k_block_sums / k_block_table3 index them; k_stream_capture fills the column store (no proposals: its mask is
// null; no region-based check of the bases: its region table is empty).  Two kernels of its own beside the mark:
//
//   k_sites_mark    one thread per site: ORs the bit of pos1 - 1 into the bitmap (an integer atomic: repeated positions
//                   set one bit, two sites of one word both land); a site behind the bitmap's span sets none
//   k_sites_eval    one thread per site: the shared column lookup, walk, genotype, germline rule and non-phased cascade
//                   (himut_column.h), the slot's read looked up for mapq where the cell is the alt allele; the record
//                   goes to recs[site] (every site has exactly one: no compaction); the counters go through LDS atomics
//                   per workgroup and one integer atomic per counter and workgroup
// (k_front_totals of the column front leaves the marked positions and column slots of the run for the host's check of the
// kept capacities)
#pragma once

#include "himut_column.h"

namespace himut {

static_assert(sizeof(himut_site_record) == 64, "himut_site_record is 64 bytes (SITE_RECORD_DTYPE of _ffi.py)");
static_assert(offsetof(himut_site_record, status) == 10 && offsetof(himut_site_record, gt) == 12 && offsetof(himut_site_record, gq) == 16 &&
              offsetof(himut_site_record, counts) == 20 && offsetof(himut_site_record, alt_bqsum) == 44 &&
              offsetof(himut_site_record, alt_mq) == 56 && offsetof(himut_site_record, reserved) == 60, "himut_site_record layout");

// the run's own scalars (unsigned long long each)
constexpr int SITES_SC_LOG = 0;        // 20 counters
constexpr int SITES_SC_NSLOTS = 20;    // column-store slots the run needs
constexpr int SITES_SC_WORDS = 32;

constexpr int SITES_LOG_SITES = 0, SITES_LOG_NOCOV = 1, SITES_LOG_GERM = 2, SITES_LOG_VERDICT = 3, SITES_LOG_ALT = 14,
              SITES_LOG_MARKED = 15;
constexpr int SITES_WG_COUNTERS = 15;  // log[0 .. 14]: what k_sites_eval counts

// pos1 >= 1 (the host checked); a site behind the span the bitmap covers marks nothing and is answered NoCoverage
__global__ void __launch_bounds__(256) k_sites_mark(const int32_t* pos1, int64_t nsites, uint32_t* bits, int64_t nwords) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nsites) return;
    const int32_t rpos = pos1[j] - 1;
    if (rpos >= 0 && (int64_t)(rpos >> 5) < nwords) atomicOr(bits + (rpos >> 5), 1u << (rpos & 31));
}

struct SitesArgs {
    Params P;
    SiteSets S;
    const GtLut* lut;
    PosIndex X;                  // nwords = 0: a batch without reads, no site has a column
    const uint16_t* colstore;
    int64_t nslots;              // capacity of colstore
    const uint8_t* mapq;         // per read
    const int32_t* pos1;
    const uint8_t* code;         // ref << 2 | alt, alleles A0 T1 G2 C3
    int64_t nsites;
    himut_site_record* recs;
    unsigned long long* sc;
    int* err;
};

#ifndef HIMUT_SITES_BATCH
#define HIMUT_SITES_BATCH 8
#endif

// the verdict's counter: log[3 .. 13] in the order HetSite .. ComSnp, LowDepth, HighDepth, PASS
__device__ __forceinline__ int sites_log_slot(int st) {
    return st == HIMUT_ST_NOCOV ? SITES_LOG_NOCOV : st == HIMUT_ST_GERMLINE ? SITES_LOG_GERM : SITES_LOG_VERDICT + verdict_rank(st);
}

// the sites run's rule for the walk: the alt reads whose mapq is at least min_mapq (the slot's read looked up)
struct SitesHook {
    const uint8_t* mapq;         // of the column's first read on
    const int alt, min_mapq;
    uint32_t alt_mq = 0;
    __device__ __forceinline__ bool keep(uint32_t, uint32_t) { return true; }
    __device__ __forceinline__ void base(uint32_t i, uint32_t cell, uint32_t) {
        if ((int)cell == alt && (int)mapq[i] >= min_mapq) alt_mq++;
    }
};

__global__ void __launch_bounds__(256, 2) k_sites_eval(SitesArgs A) {
    __shared__ double s_lut[3 * 256];
    __shared__ double s_prior[4];
    __shared__ uint32_t s_cnt[16];
    const int tid = threadIdx.x;
    stage_gt_lut(A.lut, s_lut, s_prior, tid);
    if (tid < 16) s_cnt[tid] = 0;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + tid;
    int bad = 0;
    if (j < A.nsites && !*A.err) {
        const int32_t tpos = A.pos1[j];
        const int ref = (int)(A.code[j] >> 2) & 3, alt = (int)A.code[j] & 3;
        const Column C = column_find(A.X, A.colstore, A.nslots, tpos - 1);
        if (C.ok) {
            SitesHook hook{A.mapq + C.lo, alt, A.P.p.min_mapq};
            Pile pile;
            walk_column<HIMUT_SITES_BATCH>(C, s_lut, ref, alt, A.P.p.min_bq, hook, pile, bad);
            int status = HIMUT_ST_NOCOV, gq = 0, state = 0, c0 = 0, c1 = 0;       // depth 0: no genotype is taken
            if (pile.depth() != 0) {
                const Genotyped g = genotype_column(pile, s_prior, ref);
                gq = g.gq; state = g.state; c0 = allele2char(g.g0); c1 = allele2char(g.g1);
                // a site without an alt read has alt_hi == 0: LowBQ unless an earlier rule holds
                status = is_germ_gt(g, pile, ref, alt) ? HIMUT_ST_GERMLINE : call_verdict(A.P, A.S, g, pile, tpos, ref, alt);
            }
            atomicAdd(&s_cnt[SITES_LOG_SITES], 1u);
            atomicAdd(&s_cnt[sites_log_slot(status)], 1u);
            if (pile.alt_count) atomicAdd(&s_cnt[SITES_LOG_ALT], 1u);
            uint4 w0, w1, w2, w3;
            w0.x = (uint32_t)j; w0.y = (uint32_t)tpos;
            w0.z = (uint32_t)allele2char(ref) | ((uint32_t)allele2char(alt) << 8) | ((uint32_t)status << 16) | ((uint32_t)state << 24);
            w0.w = (uint32_t)c0 | ((uint32_t)c1 << 8);
            w1.x = (uint32_t)gq; w1.y = pile.cnt[0]; w1.z = pile.cnt[1]; w1.w = pile.cnt[2];
            w2.x = pile.cnt[3]; w2.y = pile.cnt[4]; w2.z = pile.cnt[5]; w2.w = pile.alt_bq;
            w3.x = pile.ref_bq; w3.y = pile.alt_hi; w3.z = hook.alt_mq; w3.w = 0u;
            uint4* dst = reinterpret_cast<uint4*>(A.recs + j);
            dst[0] = w0; dst[1] = w1; dst[2] = w2; dst[3] = w3;
        }
    }
    if (bad) atomicOr(A.err, bad);
    __syncthreads();
    if (tid < SITES_WG_COUNTERS && s_cnt[tid]) atomicAdd(A.sc + SITES_SC_LOG + tid, (unsigned long long)s_cnt[tid]);
}

}  // namespace himut
