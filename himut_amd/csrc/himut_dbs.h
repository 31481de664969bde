// Device code of the dbs run (himut_run_dbs): somatic doublet base substitutions from the call path's pile.  The
// contract is include/himut_hip.h (himut_run_dbs) and DESIGN.md section 8, row 10.
//
// The run shares the call run's front half -- k_parse_cs under the call run's parameter block marks the substitution
// positions of the reads that pass the mapq, query-length and identity gates, k_block_sums / k_block_table3 index the
// marked positions, k_stream_capture fills the column store and leaves every read's quality sum (no proposals: its mask
// is null) -- and adds four kernels of its own:
//
//   k_dbs_propose   sixteen lanes per read over its mismatch entries: an entry that opens a run of substitutions at
//                   consecutive positions measures the run from the list itself (its neighbours are read from memory,
//                   so a run that straddles two turns of the group's loop is found like any other); a run of two that
//                   passes the read filters, the trim and the joint window and lies in a region appends a 64-bit key
//   (the keys are sorted: rocPRIM's radix sort; equal keys are one candidate, their number is n_proposers)
//   k_dbs_eval      one thread per sorted key, the first of each run of equal keys works: each half through the shared
//                   column walk, genotype, germline rule and non-phased cascade (himut_column.h) on the whole pile of
//                   its position, then both columns read by read for the joint counts; the record goes to the
//                   workgroup's first slot + its place among the workgroup's records (wg_rank): key order
//   (the shared compaction, k_compact_runs over SlotRuns<himut_dbs_record> of himut_emit.h, moves the records to the front:
//   workgroup w's start at slot w * 256)
// (k_front_totals of the column front leaves the marked positions and column slots of the run for the host's check of the
// kept capacities)
#pragma once

#include "himut_emit.h"

namespace himut {

static_assert(sizeof(himut_dbs_record) == 112, "himut_dbs_record is 112 bytes (DBS_RECORD_DTYPE of _ffi.py)");
static_assert(offsetof(himut_dbs_record, status) == 12 && offsetof(himut_dbs_record, gt_state) == 16 &&
              offsetof(himut_dbs_record, half_gq) == 24 && offsetof(himut_dbs_record, counts) == 32 &&
              offsetof(himut_dbs_record, alt_bqsum) == 80 && offsetof(himut_dbs_record, both_alt) == 88, "himut_dbs_record layout");

// the run's own scalars (unsigned long long each)
constexpr int DBS_SC_LOG = 0;        // 20 counters
constexpr int DBS_SC_NPROP = 20;     // keys k_dbs_propose wanted to append (may exceed the capacity)
constexpr int DBS_SC_NREC = 21;      // records
constexpr int DBS_SC_NSLOTS = 22;    // column-store slots the run needs
constexpr int DBS_SC_NMARKED = 23;   // marked positions
constexpr int DBS_SC_WORDS = 32;

constexpr int DBS_LOG_READS = 0, DBS_LOG_RUNS = 1, DBS_LOG_MBS = 2, DBS_LOG_TRIM = 3, DBS_LOG_WINDOW = 4, DBS_LOG_CAND = 5,
              DBS_LOG_GERM = 6, DBS_LOG_VERDICT = 7;

// key of a doublet: ascending keys = ascending (tpos, alt1, alt2), alleles in ATGC order
__device__ __forceinline__ uint64_t dbs_key(int32_t tpos, uint32_t v0, uint32_t v1) {
    return ((uint64_t)(uint32_t)tpos << 8) | ((uint64_t)(v0 & 3u) << 6) | ((uint64_t)(v1 & 3u) << 4) | ((uint64_t)((v0 >> 2) & 3u) << 2) |
           (uint64_t)((v1 >> 2) & 3u);
}

__global__ void __launch_bounds__(256) k_dbs_propose(Reads R, Derived D, Params P, const int32_t* s_start, const int32_t* s_pmaxend,
                                                     int64_t nregion, uint64_t* props, int64_t cap_props, unsigned long long* sc,
                                                     const int* err) {
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int gl = threadIdx.x & 15;
    if (r >= R.n || *err) return;
    const ReadMeta M = D.meta[r];
    if (M.flags & RF_SECONDARY) return;
    // call's read filters (caller.py:310-317), as propose_read applies them
    const int32_t qlen = R.qlen[r];
    if (!(M.flags & RF_IDENT_OK)) return;
    if (P.p.min_qv > 0 && (unsigned long long)D.bqsum[r] < (unsigned long long)P.p.min_qv * (unsigned long long)(uint32_t)qlen) return;
    if ((int)R.mapq[r] < P.p.min_mapq) return;
    if (!(P.p.qlen_lower_limit < qlen && qlen < P.p.qlen_upper_limit)) return;
    const int nm = D.nmis[r];
    const int32_t* mis = D.mis + M.segbase;
    const uint32_t* mq = D.mq + M.segbase;
    const double trim_start = floor(P.p.min_trim * (double)qlen);        // bamlib.py:226
    const double trim_end = ceil((1.0 - P.p.min_trim) * (double)qlen);   // bamlib.py:227
    const int64_t w = P.p.mismatch_window_size;
    uint32_t n_runs = 0, n_mbs = 0, n_trim = 0, n_win = 0;
    for (int e = gl; e < nm; e += 16) {
        const uint32_t v0 = mq[e];
        if (!(v0 & 16u)) continue;
        const int32_t p = mis[e];
        if (e > 0 && (mq[e - 1] & 16u) && mis[e - 1] == p - 1) continue;        // inside a run: its first entry measures it
        int len = 1;
        while (len < 3 && e + len < nm && (mq[e + len] & 16u) && mis[e + len] == p + len) len++;
        if (len == 1) continue;
        if (len > 2) { n_mbs++; continue; }
        n_runs++;
        const int64_t q = v0 >> 5;
        if ((double)q < trim_start || (double)q > trim_end || (double)(q + 1) < trim_start || (double)(q + 1) > trim_end) { n_trim++; continue; }
        int64_t s1, e1, s2, e2;
        mismatch_range(p, q, qlen, w, s1, e1);
        mismatch_range((int64_t)p + 1, q + 1, qlen, w, s2, e2);
        const int64_t ws = s1 < s2 ? s1 : s2, we = e1 > e2 ? e1 : e2;
        if ((int64_t)mismatches_in(mis, nm, ws, we) - 2 > (int64_t)P.p.max_mismatch_count) { n_win++; continue; }
        if (!in_region(s_start, s_pmaxend, nregion, p)) continue;
        const unsigned long long slot = atomicAdd(sc + DBS_SC_NPROP, 1ull);
        if ((int64_t)slot < cap_props) props[slot] = dbs_key(p, v0, mq[e + 1]);
    }
    if (gl == 0) atomicAdd(sc + DBS_SC_LOG + DBS_LOG_READS, 1ull);
    if (n_runs) atomicAdd(sc + DBS_SC_LOG + DBS_LOG_RUNS, (unsigned long long)n_runs);
    if (n_mbs) atomicAdd(sc + DBS_SC_LOG + DBS_LOG_MBS, (unsigned long long)n_mbs);
    if (n_trim) atomicAdd(sc + DBS_SC_LOG + DBS_LOG_TRIM, (unsigned long long)n_trim);
    if (n_win) atomicAdd(sc + DBS_SC_LOG + DBS_LOG_WINDOW, (unsigned long long)n_win);
}

struct DbsArgs {
    Params P;
    SiteSets S;
    const GtLut* lut;
    PosIndex X;
    const uint16_t* colstore;
    int64_t nslots;              // capacity of colstore
    const uint64_t* keys;        // sorted
    int64_t nkeys;
    himut_dbs_record* recs;      // workgroup w's records start at w * 256
    uint32_t* wgcnt;             // records per workgroup
    unsigned long long* sc;
    int* err;
};

#ifndef HIMUT_DBS_BATCH
#define HIMUT_DBS_BATCH 8
#endif

struct DbsHalf {
    int status;                  // HIMUT_ST_*; -1: dropped as germline
    Genotyped g;
    Pile pile;
};

// The verdict call's non-phased cascade (caller.py:332-550) gives (tpos, ref, alt) on the whole pile of the position:
// no chunk edge and no vote, so the walk has no rule of its own.
__device__ __forceinline__ DbsHalf dbs_half(const DbsArgs& A, const double* s_lut, const double* s_prior, const Column& C,
                                            const int32_t tpos, const int ref, const int alt, int& bad) {
    DbsHalf h;
    NoHook hook;
    walk_column<HIMUT_DBS_BATCH>(C, s_lut, ref, alt, A.P.p.min_bq, hook, h.pile, bad);
    h.g = genotype_column(h.pile, s_prior, ref);
    h.status = is_germ_gt(h.g, h.pile, ref, alt) ? -1 : call_verdict(A.P, A.S, h.g, h.pile, tpos, ref, alt);
    return h;
}

// the verdict's counter: log[7 .. 17] in the order HetSite .. ComSnp, LowDepth, HighDepth, PASS
__device__ __forceinline__ int dbs_log_slot(int st) { return DBS_LOG_VERDICT + verdict_rank(st); }

__global__ void __launch_bounds__(256, 2) k_dbs_eval(DbsArgs A) {
    __shared__ double s_lut[3 * 256];
    __shared__ double s_prior[4];
    __shared__ int s_e[4];
    const int tid = threadIdx.x;
    stage_gt_lut(A.lut, s_lut, s_prior, tid);
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + tid;
    bool emit = false;
    int bad = 0;
    uint4 w0 = make_uint4(0, 0, 0, 0), w1 = w0, w2 = w0, w3 = w0, w4 = w0, w5 = w0, w6 = w0;
    if (j < A.nkeys && !*A.err) {
        const uint64_t key = A.keys[j];
        if (j == 0 || A.keys[j - 1] != key) {                // the first of its run of equal keys: the candidate
            uint32_t n_prop = 1;
            while (j + n_prop < A.nkeys && A.keys[j + n_prop] == key) n_prop++;
            const int32_t tpos = (int32_t)(key >> 8);
            const int alt0 = (int)((key >> 6) & 3u), alt1 = (int)((key >> 4) & 3u), ref0 = (int)((key >> 2) & 3u), ref1 = (int)(key & 3u);
            const Column C0 = column_find(A.X, A.colstore, A.nslots, tpos - 1), C1 = column_find(A.X, A.colstore, A.nslots, tpos);
            if (C0.ok && C1.ok && C0.n && C1.n) {                // (n = 0: not marked.  A proposer's read marked both.)
                atomicAdd(A.sc + DBS_SC_LOG + DBS_LOG_CAND, 1ull);
                const DbsHalf h0 = dbs_half(A, s_lut, s_prior, C0, tpos, ref0, alt0, bad);
                const DbsHalf h1 = dbs_half(A, s_lut, s_prior, C1, tpos + 1, ref1, alt1, bad);
                if (h0.status < 0 || h1.status < 0) atomicAdd(A.sc + DBS_SC_LOG + DBS_LOG_GERM, 1ull);
                else {
                    // ---- the joint counts: both columns read by read (two blocks of the column index: two windows)
                    const int32_t rlo = min(C0.lo, C1.lo), rhi = max(C0.lo + (int32_t)C0.n, C1.lo + (int32_t)C1.n);
                    uint32_t both_alt = 0, both_ref = 0, one_alt = 0;
                    constexpr int EB = HIMUT_DBS_BATCH;
                    for (int32_t r0 = rlo; r0 < rhi; r0 += EB) {
                        uint32_t va[EB], vb[EB];
#pragma unroll
                        for (int k = 0; k < EB; k++) {
                            const int32_t r = r0 + k;
                            const bool in0 = r < rhi && r >= C0.lo && r < C0.lo + (int32_t)C0.n;
                            const bool in1 = r < rhi && r >= C1.lo && r < C1.lo + (int32_t)C1.n;
                            va[k] = in0 ? (uint32_t)C0.col[(int64_t)(r - C0.lo) * C0.stride] : (uint32_t)CELL_EMPTY;
                            vb[k] = in1 ? (uint32_t)C1.col[(int64_t)(r - C1.lo) * C1.stride] : (uint32_t)CELL_EMPTY;
                        }
#pragma unroll
                        for (int k = 0; k < EB; k++) {
                            const int a = (int)(va[k] & 7u), b = (int)(vb[k] & 7u);      // (4, 5, 7: no allele there)
                            const bool a_alt = a == alt0, b_alt = b == alt1;
                            if (a_alt && b_alt) both_alt++;
                            else if (a_alt || b_alt) one_alt++;
                            if (a == ref0 && b == ref1) both_ref++;
                        }
                    }
                    // a verdict ahead of LowDepth in either half: the earlier one; else the joint counts decide
                    const int k0 = verdict_rank(h0.status), k1 = verdict_rank(h1.status);
                    int status;
                    if (k0 < 8 || k1 < 8) status = k0 <= k1 ? h0.status : h1.status;
                    else if ((int64_t)both_ref < A.P.p.min_ref_count || (int64_t)both_alt < A.P.p.min_alt_count) status = HIMUT_ST_LOWDEPTH;
                    else if (h0.status == HIMUT_ST_HIGHDEPTH || h1.status == HIMUT_ST_HIGHDEPTH) status = HIMUT_ST_HIGHDEPTH;
                    else status = HIMUT_ST_PASS;
                    atomicAdd(A.sc + DBS_SC_LOG + dbs_log_slot(status), 1ull);
                    emit = true;
                    w0.x = (uint32_t)tpos; w0.y = (uint32_t)min(h0.g.gq, h1.g.gq);
                    w0.z = (uint32_t)allele2char(ref0) | ((uint32_t)allele2char(ref1) << 8) | ((uint32_t)allele2char(alt0) << 16) |
                           ((uint32_t)allele2char(alt1) << 24);
                    w0.w = (uint32_t)(status & 255) | ((uint32_t)(h0.status & 255) << 8) | ((uint32_t)(h1.status & 255) << 16);
                    w1.x = (uint32_t)h0.g.state | ((uint32_t)h1.g.state << 8) | ((uint32_t)allele2char(h0.g.g0) << 16) |
                           ((uint32_t)allele2char(h0.g.g1) << 24);
                    w1.y = (uint32_t)allele2char(h1.g.g0) | ((uint32_t)allele2char(h1.g.g1) << 8);
                    w1.z = (uint32_t)h0.g.gq; w1.w = (uint32_t)h1.g.gq;
                    const uint32_t *c0 = h0.pile.cnt, *c1 = h1.pile.cnt;
                    w2.x = c0[0]; w2.y = c0[1]; w2.z = c0[2]; w2.w = c0[3];
                    w3.x = c0[4]; w3.y = c0[5]; w3.z = c1[0]; w3.w = c1[1];
                    w4.x = c1[2]; w4.y = c1[3]; w4.z = c1[4]; w4.w = c1[5];
                    w5.x = h0.pile.alt_bq; w5.y = h1.pile.alt_bq; w5.z = both_alt; w5.w = both_ref;
                    w6.x = one_alt; w6.y = n_prop;
                }
            }
        }
    }
    // ---- the workgroup's records in thread (= key) order
    const WgRank e = wg_rank<4>(emit, s_e);
    if (emit) {
        uint4* dst = reinterpret_cast<uint4*>(A.recs + ((int64_t)blockIdx.x * 256 + e.rank));
        dst[0] = w0; dst[1] = w1; dst[2] = w2; dst[3] = w3; dst[4] = w4; dst[5] = w5; dst[6] = w6;
    }
    if (bad) atomicOr(A.err, bad);
    if (tid == 0) A.wgcnt[blockIdx.x] = (uint32_t)e.total;
}

}  // namespace himut
