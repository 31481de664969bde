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
//   k_dbs_eval      one thread per sorted key, the first of each run of equal keys works: both columns' slots in fetch
//                   order (counts, the three ordered fp64 sums per allele, the shared genotype(), the non-phased
//                   cascade of k_eval_columns per half), then both columns read by read for the joint counts; the
//                   record goes to the workgroup's first slot + its place among the workgroup's records (a ballot):
//                   key order
//   k_dbs_compact   every workgroup adds up the record counts in front of it and moves its run of records there
//   k_dbs_totals    the marked positions and column slots of the run, for the host's check of the kept capacities
#pragma once

#include "himut_device.h"

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

// start <= tpos <= end for some region
__device__ __forceinline__ bool dbs_in_region(const int32_t* s_start, const int32_t* s_pmaxend, int64_t nregion, int32_t tpos) {
    const int64_t k = upper_bound(s_start, (int64_t)0, nregion, tpos);
    return k > 0 && s_pmaxend[k - 1] >= tpos;
}

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
        int lo = 0, hi = nm;                                 // bisect_left(ws)
        while (lo < hi) { const int m = (lo + hi) >> 1; if ((int64_t)mis[m] < ws) lo = m + 1; else hi = m; }
        int up = lo;                                         // bisect_right(we)
        hi = nm;
        while (up < hi) { const int m = (up + hi) >> 1; if (we < (int64_t)mis[m]) hi = m; else up = m + 1; }
        if ((int64_t)(up - lo) - 2 > (int64_t)P.p.max_mismatch_count) { n_win++; continue; }
        if (!dbs_in_region(s_start, s_pmaxend, nregion, p)) continue;
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

// a column of the store: the slot of read lo + i is col[i * stride]
struct DbsColumn {
    const uint16_t* col;
    uint32_t n, stride;
    int32_t lo;
    bool ok;                     // marked, and inside the store's capacity
};

__device__ __forceinline__ DbsColumn dbs_column(const DbsArgs& A, int32_t rpos) {
    DbsColumn c;
    c.col = A.colstore; c.n = 0; c.stride = 0; c.lo = 0; c.ok = false;
    if (rpos < 0 || (int64_t)(rpos >> 5) >= A.X.nwords || !((A.X.bits[rpos >> 5] >> (rpos & 31)) & 1u)) return c;
    const uint32_t u = pos_rank(A.X, rpos);
    const BlockTab bt = A.X.bt[rpos >> 8];
    c.n = bt.ncnt & BT_N_MASK; c.stride = bt.ncnt >> 22; c.lo = bt.lo;
    const int64_t first = (int64_t)bt.boff + (int64_t)(u - bt.ufirst);
    // a column past the capacity kept from an earlier run: the host runs again with exact sizes
    c.ok = !(c.n && first + (int64_t)(c.n - 1) * (int64_t)c.stride >= A.nslots);
    c.col = A.colstore + first;
    return c;
}

struct DbsHalf {
    int status;                  // HIMUT_ST_*; -1: dropped as germline
    int gq, state, g0, g1;
    uint32_t cnt[6];
    uint32_t altq;               // the alt allele's quality sum
};

#ifndef HIMUT_DBS_BATCH
#define HIMUT_DBS_BATCH 8
#endif

// The verdict call's non-phased cascade (caller.py:332-550) gives (tpos, ref, alt) on the whole pile of the position:
// k_eval_columns without its chunk edge and without the vote.
__device__ __forceinline__ DbsHalf dbs_half(const DbsArgs& A, const double* s_lut, const double* s_prior, const DbsColumn& C,
                                            const int32_t tpos, const int ref, const int alt, int& bad) {
    const int min_bq = A.P.p.min_bq;
    uint32_t cnt[6] = {0, 0, 0, 0, 0, 0};
    GtSums S;
#pragma unroll
    for (int b = 0; b < 4; b++) { S[0][b] = 0.0; S[1][b] = 0.0; S[2][b] = 0.0; }
    uint32_t ref_count = 0, alt_count = 0, alt_hi = 0, Aq = 0;
    double R0 = 0.0, R1 = 0.0, R2 = 0.0, A0 = 0.0, A1 = 0.0, A2 = 0.0;
    constexpr int EB = HIMUT_DBS_BATCH;
    const uint32_t n = C.n, stride = C.stride;
    for (uint32_t i0 = 0; i0 < n; i0 += EB) {    // EB slots in flight: their addresses do not depend on each other
        uint32_t vv[EB];
#pragma unroll
        for (int k = 0; k < EB; k++) vv[k] = (i0 + k < n) ? (uint32_t)C.col[(int64_t)(i0 + k) * stride] : (uint32_t)CELL_EMPTY;
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
                    ref_count++;
                    R0 = R0 + vh; R1 = R1 + vt; R2 = R2 + ve;
                } else if ((int)cell == alt) {
                    alt_count++; Aq += q; if ((int)q >= min_bq) alt_hi++;      // caller.py:160-171
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
    const Genotype gt = genotype(S, s_prior, ref);
    int g0 = (int)HIMUT_GT_B1(gt.best), g1 = (int)HIMUT_GT_B2(gt.best);
    const int state = gt_state_of(g0, g1, ref);
    if (g0 != ref && ((g0 == ref) + (g1 == ref)) == 1) { int tmp = g0; g0 = g1; g1 = tmp; }  // gtlib.py:133-134
    const uint32_t depth = cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[5];  // bamlib.py:213-219
    bool germ;  // caller.py:111-147
    if (state == 1) germ = (g0 == ref && g1 == alt);
    else if (state == 2) {
        uint32_t c0 = 0, c1 = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) { if (g0 == b) c0 = cnt[b]; if (g1 == b) c1 = cnt[b]; }
        germ = ((cnt[0] + cnt[1] + cnt[2] + cnt[3]) == (c0 + c1)) && (alt == g0 || alt == g1);
    } else if (state == 3) germ = (ref_count == 0) && (g0 == alt && g1 == alt);
    else germ = (alt == g0);
    int status;
    if (germ) status = -1;
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
    DbsHalf h;
    h.status = status; h.gq = gt.gq; h.state = state; h.g0 = g0; h.g1 = g1; h.altq = Aq;
#pragma unroll
    for (int b = 0; b < 6; b++) h.cnt[b] = cnt[b];
    return h;
}

// place of a half verdict in the order of precedence between the halves; 8: none of the eight
__device__ __forceinline__ int dbs_precedence(int st) {
    return st == HIMUT_ST_HET ? 0 : st == HIMUT_ST_HETALT ? 1 : st == HIMUT_ST_HOMALT ? 2 : st == HIMUT_ST_INDEL ? 3 :
           st == HIMUT_ST_LOWGQ ? 4 : st == HIMUT_ST_LOWBQ ? 5 : st == HIMUT_ST_PON ? 6 : st == HIMUT_ST_COMSNP ? 7 : 8;
}
// the verdict's counter: log[7 ..17] in the order HetSite .. ComSnp, LowDepth, HighDepth, PASS
__device__ __forceinline__ int dbs_log_slot(int st) {
    const int k = dbs_precedence(st);
    return DBS_LOG_VERDICT + (k < 8 ? k : st == HIMUT_ST_LOWDEPTH ? 8 : st == HIMUT_ST_HIGHDEPTH ? 9 : 10);
}

__global__ void __launch_bounds__(256, 2) k_dbs_eval(DbsArgs A) {
    __shared__ double s_lut[3 * 256];
    __shared__ double s_prior[4];
    __shared__ int s_e[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < 3 * 256; i += 256) s_lut[i] = A.lut->t[i >> 8][i & 255];
    if (tid < 4) s_prior[tid] = A.lut->prior[tid];
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
            const DbsColumn C0 = dbs_column(A, tpos - 1), C1 = dbs_column(A, tpos);
            if (C0.ok && C1.ok) {
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
                    const int k0 = dbs_precedence(h0.status), k1 = dbs_precedence(h1.status);
                    int status;
                    if (k0 < 8 || k1 < 8) status = k0 <= k1 ? h0.status : h1.status;
                    else if ((int64_t)both_ref < A.P.p.min_ref_count || (int64_t)both_alt < A.P.p.min_alt_count) status = HIMUT_ST_LOWDEPTH;
                    else if (h0.status == HIMUT_ST_HIGHDEPTH || h1.status == HIMUT_ST_HIGHDEPTH) status = HIMUT_ST_HIGHDEPTH;
                    else status = HIMUT_ST_PASS;
                    atomicAdd(A.sc + DBS_SC_LOG + dbs_log_slot(status), 1ull);
                    emit = true;
                    w0.x = (uint32_t)tpos; w0.y = (uint32_t)min(h0.gq, h1.gq);
                    w0.z = (uint32_t)allele2char(ref0) | ((uint32_t)allele2char(ref1) << 8) | ((uint32_t)allele2char(alt0) << 16) |
                           ((uint32_t)allele2char(alt1) << 24);
                    w0.w = (uint32_t)(status & 255) | ((uint32_t)(h0.status & 255) << 8) | ((uint32_t)(h1.status & 255) << 16);
                    w1.x = (uint32_t)h0.state | ((uint32_t)h1.state << 8) | ((uint32_t)allele2char(h0.g0) << 16) | ((uint32_t)allele2char(h0.g1) << 24);
                    w1.y = (uint32_t)allele2char(h1.g0) | ((uint32_t)allele2char(h1.g1) << 8);
                    w1.z = (uint32_t)h0.gq; w1.w = (uint32_t)h1.gq;
                    w2.x = h0.cnt[0]; w2.y = h0.cnt[1]; w2.z = h0.cnt[2]; w2.w = h0.cnt[3];
                    w3.x = h0.cnt[4]; w3.y = h0.cnt[5]; w3.z = h1.cnt[0]; w3.w = h1.cnt[1];
                    w4.x = h1.cnt[2]; w4.y = h1.cnt[3]; w4.z = h1.cnt[4]; w4.w = h1.cnt[5];
                    w5.x = h0.altq; w5.y = h1.altq; w5.z = both_alt; w5.w = both_ref;
                    w6.x = one_alt; w6.y = n_prop;
                }
            }
        }
    }
    // ---- the workgroup's records in thread (= key) order
    const unsigned long long eb = __ballot(emit);
    if (lane == 0) s_e[wv] = __popcll(eb);
    __syncthreads();
    int place = (int)__popcll(eb & ((1ULL << lane) - 1ULL));
    for (int k = 0; k < wv; k++) place += s_e[k];
    if (emit) {
        uint4* dst = reinterpret_cast<uint4*>(A.recs + ((int64_t)blockIdx.x * 256 + place));
        dst[0] = w0; dst[1] = w1; dst[2] = w2; dst[3] = w3; dst[4] = w4; dst[5] = w5; dst[6] = w6;
    }
    if (bad) atomicOr(A.err, bad);
    if (tid == 0) A.wgcnt[blockIdx.x] = (uint32_t)(s_e[0] + s_e[1] + s_e[2] + s_e[3]);
}

// Workgroup w's records (wgcnt[w] of them, from slot w * 256 on) to their place behind the records of the workgroups in
// front of it; the last workgroup leaves the record count.
__global__ void __launch_bounds__(256) k_dbs_compact(const himut_dbs_record* recs, const uint32_t* wgcnt, himut_dbs_record* out,
                                                     unsigned long long* sc) {
    __shared__ unsigned long long s_sum[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned long long part = 0;
    for (int64_t k = tid; k < (int64_t)blockIdx.x; k += 256) part += wgcnt[k];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d, 64);
    if (lane == 0) s_sum[wv] = part;
    __syncthreads();
    const unsigned long long base = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    const uint32_t mine = min(wgcnt[blockIdx.x], 256u);
    const uint4* src = reinterpret_cast<const uint4*>(recs + (int64_t)blockIdx.x * 256);
    uint4* dst = reinterpret_cast<uint4*>(out + base);
    for (int64_t k = tid; k < (int64_t)mine * 7; k += 256) dst[k] = src[k];
    if (blockIdx.x == gridDim.x - 1 && tid == 0) sc[DBS_SC_NREC] = base + mine;
}

// what the host compares with the kept capacities: the marked positions and the column-store slots of the run
__global__ void k_dbs_totals(PosIndex X, const uint32_t* blkoff, const uint32_t* blkslots, unsigned long long* sc) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const BlockTab t = X.bt[X.nblk - 1];
    sc[DBS_SC_NMARKED] = (unsigned long long)t.ufirst + (unsigned long long)(t.ncnt >> 22);
    sc[DBS_SC_NSLOTS] = (unsigned long long)blkoff[X.nblk - 1] + (unsigned long long)blkslots[X.nblk - 1];
}

}  // namespace himut
