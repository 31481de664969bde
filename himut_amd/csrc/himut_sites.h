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
//   k_sites_eval    one thread per site: the column's slots several in flight, in fetch order (counts, the three ordered
//                   fp64 sums per allele with the reference and alt alleles in accumulators of their own, the slot's
//                   read looked up for mapq where the cell is the alt allele), the shared genotype(), is_germ_gt, call's
//                   non-phased cascade; the record goes to recs[site] (every site has exactly one: no compaction); the
//                   counters go through LDS atomics per workgroup and one integer atomic per counter and workgroup
//   k_sites_totals  the marked positions and column slots of the run, for the host's check of the kept capacities
//
// The column lookup and the cascade restate dbs_column / dbs_half (himut_dbs.h): that header holds the dbs kernels
// themselves, which are compiled with himut_dbs.hip alone.
#pragma once

#include "himut_device.h"

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
    const int k = st == HIMUT_ST_HET ? 0 : st == HIMUT_ST_HETALT ? 1 : st == HIMUT_ST_HOMALT ? 2 : st == HIMUT_ST_INDEL ? 3 :
                  st == HIMUT_ST_LOWGQ ? 4 : st == HIMUT_ST_LOWBQ ? 5 : st == HIMUT_ST_PON ? 6 : st == HIMUT_ST_COMSNP ? 7 :
                  st == HIMUT_ST_LOWDEPTH ? 8 : st == HIMUT_ST_HIGHDEPTH ? 9 : 10;
    return st == HIMUT_ST_NOCOV ? SITES_LOG_NOCOV : st == HIMUT_ST_GERMLINE ? SITES_LOG_GERM : SITES_LOG_VERDICT + k;
}

__global__ void __launch_bounds__(256, 2) k_sites_eval(SitesArgs A) {
    __shared__ double s_lut[3 * 256];
    __shared__ double s_prior[4];
    __shared__ uint32_t s_cnt[16];
    const int tid = threadIdx.x;
    for (int i = tid; i < 3 * 256; i += 256) s_lut[i] = A.lut->t[i >> 8][i & 255];
    if (tid < 4) s_prior[tid] = A.lut->prior[tid];
    if (tid < 16) s_cnt[tid] = 0;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + tid;
    int bad = 0;
    if (j < A.nsites && !*A.err) {
        const int32_t tpos = A.pos1[j], rpos = tpos - 1;
        const int ref = (int)(A.code[j] >> 2) & 3, alt = (int)A.code[j] & 3;
        // ---- the column (dbs_column): marked, and inside the store's capacity
        const uint16_t* col = A.colstore;
        uint32_t n = 0, stride = 0;
        int32_t lo = 0;
        bool ok = true;
        if (rpos >= 0 && (int64_t)(rpos >> 5) < A.X.nwords && ((A.X.bits[rpos >> 5] >> (rpos & 31)) & 1u)) {
            const uint32_t u = pos_rank(A.X, rpos);
            const BlockTab bt = A.X.bt[rpos >> 8];
            n = bt.ncnt & BT_N_MASK; stride = bt.ncnt >> 22; lo = bt.lo;
            const int64_t first = (int64_t)bt.boff + (int64_t)(u - bt.ufirst);
            // a column past the capacity kept from an earlier run: the host runs again with exact sizes
            ok = !(n && first + (int64_t)(n - 1) * (int64_t)stride >= A.nslots);
            col = A.colstore + first;
        }
        if (ok) {
            const int min_bq = A.P.p.min_bq, min_mapq = A.P.p.min_mapq;
            uint32_t cnt[6] = {0, 0, 0, 0, 0, 0};
            GtSums S;
#pragma unroll
            for (int b = 0; b < 4; b++) { S[0][b] = 0.0; S[1][b] = 0.0; S[2][b] = 0.0; }
            uint32_t ref_count = 0, alt_count = 0, alt_hi = 0, alt_mq = 0, Aq = 0, Rq = 0;
            double R0 = 0.0, R1 = 0.0, R2 = 0.0, A0 = 0.0, A1 = 0.0, A2 = 0.0;
            constexpr int EB = HIMUT_SITES_BATCH;
            for (uint32_t i0 = 0; i0 < n; i0 += EB) {    // EB slots in flight: their addresses do not depend on each other
                uint32_t vv[EB];
#pragma unroll
                for (int k = 0; k < EB; k++) vv[k] = (i0 + k < n) ? (uint32_t)col[(int64_t)(i0 + k) * stride] : (uint32_t)CELL_EMPTY;
#pragma unroll
                for (int k = 0; k < EB; k++) {
                    const uint32_t v = vv[k];
                    const uint32_t cell = v & 7u;
                    if ((v & 15u) == CELL_EMPTY) continue;
                    if (v & CELL_INS) cnt[4]++;
                    if (cell < 4) {
                        const uint32_t q = v >> 8;
                        if (q == 0) bad |= 1 << HIMUT_ERR_BQ0;                     // gtlib.py:64
                        const double vh = s_lut[q], vt = s_lut[256 + q], ve = s_lut[512 + q];
                        if ((int)cell == ref) {
                            ref_count++; Rq += q;
                            R0 = R0 + vh; R1 = R1 + vt; R2 = R2 + ve;
                        } else if ((int)cell == alt) {
                            alt_count++; Aq += q; if ((int)q >= min_bq) alt_hi++;      // caller.py:160-171
                            if ((int)A.mapq[(int64_t)lo + (int64_t)(i0 + k)] >= min_mapq) alt_mq++;   // the slot's read
                            A0 = A0 + vh; A1 = A1 + vt; A2 = A2 + ve;
                        } else {
#pragma unroll
                            for (int b = 0; b < 4; b++) {
                                if ((int)cell == b) {
                                    cnt[b]++;
                                    S[0][b] = S[0][b] + vh;
                                    S[1][b] = S[1][b] + vt;
                                    S[2][b] = S[2][b] + ve;
                                }
                            }
                        }
                    } else if (cell == CELL_DEL) cnt[5]++;
                    else if (cell == CELL_OTHER) bad |= 1 << HIMUT_ERR_BASE;       // caller.py:57
                }
            }
#pragma unroll
            for (int b = 0; b < 4; b++) {
                if (b == ref) { cnt[b] = ref_count; S[0][b] = R0; S[1][b] = R1; S[2][b] = R2; }
                if (b == alt) { cnt[b] = alt_count; S[0][b] = A0; S[1][b] = A1; S[2][b] = A2; }
            }
            const uint32_t depth = cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[5];  // bamlib.py:213-219
            int status = HIMUT_ST_NOCOV, gq = 0, state = 0, c0 = 0, c1 = 0;       // depth 0: no genotype is taken
            if (depth != 0) {
                const Genotype gt = genotype(S, s_prior, ref);
                int g0 = (int)HIMUT_GT_B1(gt.best), g1 = (int)HIMUT_GT_B2(gt.best);
                state = gt_state_of(g0, g1, ref);
                if (g0 != ref && ((g0 == ref) + (g1 == ref)) == 1) { int tmp = g0; g0 = g1; g1 = tmp; }  // gtlib.py:133-134
                gq = gt.gq; c0 = allele2char(g0); c1 = allele2char(g1);
                bool germ;  // caller.py:111-147
                if (state == 1) germ = (g0 == ref && g1 == alt);
                else if (state == 2) {
                    uint32_t n0 = 0, n1 = 0;
#pragma unroll
                    for (int b = 0; b < 4; b++) { if (g0 == b) n0 = cnt[b]; if (g1 == b) n1 = cnt[b]; }
                    germ = ((cnt[0] + cnt[1] + cnt[2] + cnt[3]) == (n0 + n1)) && (alt == g0 || alt == g1);
                } else if (state == 3) germ = (ref_count == 0) && (g0 == alt && g1 == alt);
                else germ = (alt == g0);
                // call's non-phased cascade (caller.py:332-550), as dbs_half states it; a site without an alt read has
                // alt_hi == 0: LowBQ unless an earlier rule holds
                if (germ) status = HIMUT_ST_GERMLINE;
                else if (state == 1) status = HIMUT_ST_HET;
                else if (state == 2) status = HIMUT_ST_HETALT;
                else if (state == 3) status = HIMUT_ST_HOMALT;
                else if (cnt[5] != 0 || cnt[4] != 0) status = HIMUT_ST_INDEL;
                else if (gt.gq < A.P.p.min_gq) status = HIMUT_ST_LOWGQ;
                else if (alt_hi == 0) status = HIMUT_ST_LOWBQ;
                else {
                    const uint64_t key = ((uint64_t)(uint32_t)tpos << 4) | ((uint64_t)ref << 2) | (uint64_t)alt;
                    const SiteSets& St = A.S;
                    const bool site_maybe = (int64_t)tpos < St.nposbits && ((St.posbits[tpos >> 5] >> (tpos & 31)) & 1u);
                    if (site_maybe && key_in(St.pon, St.npon, key)) status = HIMUT_ST_PON;
                    else if (site_maybe && key_in(St.com, St.ncom, key)) status = HIMUT_ST_COMSNP;
                    else if (!((int64_t)ref_count >= A.P.p.min_ref_count && (int64_t)alt_count >= A.P.p.min_alt_count)) status = HIMUT_ST_LOWDEPTH;
                    else if ((int64_t)depth > A.P.p.md_threshold) status = HIMUT_ST_HIGHDEPTH;
                    else status = HIMUT_ST_PASS;
                }
            }
            atomicAdd(&s_cnt[SITES_LOG_SITES], 1u);
            atomicAdd(&s_cnt[sites_log_slot(status)], 1u);
            if (alt_count) atomicAdd(&s_cnt[SITES_LOG_ALT], 1u);
            uint4 w0, w1, w2, w3;
            w0.x = (uint32_t)j; w0.y = (uint32_t)tpos;
            w0.z = (uint32_t)allele2char(ref) | ((uint32_t)allele2char(alt) << 8) | ((uint32_t)status << 16) | ((uint32_t)state << 24);
            w0.w = (uint32_t)c0 | ((uint32_t)c1 << 8);
            w1.x = (uint32_t)gq; w1.y = cnt[0]; w1.z = cnt[1]; w1.w = cnt[2];
            w2.x = cnt[3]; w2.y = cnt[4]; w2.z = cnt[5]; w2.w = Aq;
            w3.x = Rq; w3.y = alt_hi; w3.z = alt_mq; w3.w = 0u;
            uint4* dst = reinterpret_cast<uint4*>(A.recs + j);
            dst[0] = w0; dst[1] = w1; dst[2] = w2; dst[3] = w3;
        }
    }
    if (bad) atomicOr(A.err, bad);
    __syncthreads();
    if (tid < SITES_WG_COUNTERS && s_cnt[tid]) atomicAdd(A.sc + SITES_SC_LOG + tid, (unsigned long long)s_cnt[tid]);
}

// what the host compares with the kept capacity, and the run's last counter: the column-store slots and the marked
// positions of the run
__global__ void k_sites_totals(PosIndex X, const uint32_t* blkoff, const uint32_t* blkslots, unsigned long long* sc) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const BlockTab t = X.bt[X.nblk - 1];
    sc[SITES_SC_LOG + SITES_LOG_MARKED] = (unsigned long long)t.ufirst + (unsigned long long)(t.ncnt >> 22);
    sc[SITES_SC_NSLOTS] = (unsigned long long)blkoff[X.nblk - 1] + (unsigned long long)blkslots[X.nblk - 1];
}

}  // namespace himut
