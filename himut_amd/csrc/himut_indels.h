// Device code of the indels run (himut_run_indels): germline short insertions and deletions from the decoded reads.  The
// contract is include/himut_hip.h (himut_run_indels) and DESIGN.md section 8, row 12.
//
// Everything the run needs is in HBM behind the cs decode (k_parse_cs under a parameter block whose gates are open): the
// reads' segments, SEQ, the reference string.  No bitmap, no column store, no capture.  Its own kernels:
//
//   k_indel_events  sixteen lanes per pile read over its segments (a read with more segments than lanes takes turns): a
//                   deletion segment is a deletion, SEG_INS on a segment is an insertion in front of it whose bases are the
//                   query gap behind the previous segment; the edge, length and base rules; the left shift against the
//                   reference string; an event whose anchor lies in a region appends a 64-bit key and 32 bytes
//   (the keys are sorted with the events' indices: rocPRIM's radix sort, by anchor, type and length)
//   k_indel_order   one thread per sorted key: its place among the events of equal key by (inserted bases, read), which
//                   makes the order exact; and whether it is its read's first event of the anchor
//   k_indel_eval    one thread per ordered event, the first of an allele works: n_alt and n_other from the runs around it,
//                   DP from the read window of the anchor's block, the three-state genotype in fp64, the cascade; the
//                   record goes to the workgroup's first slot + its place among the workgroup's records (wg_rank)
//   (the shared compaction, k_compact_runs over SlotRuns<himut_indel_record> of himut_emit.h, moves the records to the front)
//
// The indelcal run (himut_indelcal.h) works on the same ordered events.  What it shares with k_indel_eval is here: what the
// first event of an allele counts around itself (allele_tally) and the class of an allele against the homopolymer run
// behind its anchor (allele_class).  himut_indelcal.hip includes this file for the types and the
// device functions alone (HIMUT_INDELS_NO_KERNELS): the kernels below belong to himut_indels.hip, which launches them for
// both runs (indel_front_run).
#pragma once

#include "himut_emit.h"

namespace himut {

static_assert(sizeof(himut_indel_record) == 64, "himut_indel_record is 64 bytes (INDEL_RECORD_DTYPE of _ffi.py)");
static_assert(offsetof(himut_indel_record, type) == 8 && offsetof(himut_indel_record, gq) == 12 && offsetof(himut_indel_record, dp) == 16 &&
              offsetof(himut_indel_record, bases) == 32 && offsetof(himut_indel_record, reserved) == 48, "himut_indel_record layout");
static_assert(sizeof(himut_indel_params) == 80, "himut_indel_params is 80 bytes (IndelParams of _ffi.py)");

// the run's own scalars (unsigned long long each)
constexpr int IND_SC_LOG = 0;        // 13 counters (the first, the events, is the host's: IND_SC_NEV of a run that fits)
constexpr int IND_SC_NEV = 16;       // events k_indel_events wanted to append (may exceed the capacity)
constexpr int IND_SC_NREC = 17;      // records
constexpr int IND_SC_SOM = 18;       // the sindels run's five event counters (k_indel_events<SomRules>; IND_SOM_*)
constexpr int IND_SC_WORDS = 32;
constexpr int IND_STAGE = 512;       // events a workgroup of k_indel_events stages in LDS (16 KB)

constexpr int IND_LOG_EVENTS = 0, IND_LOG_ALLELES = 1, IND_LOG_EDGE = 2, IND_LOG_LONG = 3, IND_LOG_NBASE = 4, IND_LOG_DUP = 5,
              IND_LOG_STATE = 6, IND_LOG_PASS = 9, IND_LOG_LOWGQ = 10, IND_LOG_LOWDEPTH = 11, IND_LOG_HIGHDEPTH = 12, IND_NLOG = 13;

constexpr int IND_SOM_EVENTS = 0, IND_SOM_TRIM = 1, IND_SOM_WINDOW = 2, IND_SOM_LOWBQ = 3, IND_SOM_PROPOSING = 4, IND_NSOM = 5;

// key of an event: ascending keys = ascending (anchor, deletions before insertions, length)
constexpr int IND_KEY_SHIFT = 7;
__device__ __forceinline__ uint64_t indel_key(int32_t anchor, int type, int len) {
    return ((uint64_t)(uint32_t)anchor << IND_KEY_SHIFT) | ((uint64_t)type << 6) | (uint64_t)(len - 1);
}

// An event.  s0, s1: the inserted bases as 2-bit codes (A T G C), base i of the first 32 at bits 62 - 2i of s0, the rest
// likewise in s1, zeros behind the last: equal lengths compare as the strings do.
struct IndelEvent {
    uint64_t key, s0, s1;
    uint32_t read;
    uint32_t first;              // bit 0, k_indel_order: the read's first event at this anchor; bit 1, the sindels run's
                                 // k_indel_events: the event proposes its allele (EV_PROPOSES; 0 in every other run)
};
constexpr uint32_t EV_FIRST = 1u, EV_PROPOSES = 2u;
static_assert(sizeof(IndelEvent) == 32, "an event is two 16-byte words");

__device__ __forceinline__ uint64_t ins_keep(int n) { return n <= 0 ? 0ull : (n >= 32 ? ~0ull : (~0ull << (64 - 2 * n))); }
__device__ __forceinline__ int ins_base(uint64_t s0, uint64_t s1, int i) {
    return (int)(((i < 32 ? s0 : s1) >> (62 - 2 * (i & 31))) & 3ull);
}
// (s0, s1) < (t0, t1), then the read
__device__ __forceinline__ bool event_less(const IndelEvent& a, const IndelEvent& b) {
    if (a.s0 != b.s0) return a.s0 < b.s0;
    if (a.s1 != b.s1) return a.s1 < b.s1;
    return a.read < b.read;
}
__device__ __forceinline__ bool same_allele(const IndelEvent& a, const IndelEvent& b) { return a.key == b.key && a.s0 == b.s0 && a.s1 == b.s1; }

struct IndelArgs {
    himut_indel_params p;
    Reads R;
    Derived D;
    const uint8_t* refseq;
    int64_t reflen;
    const int32_t *s_start, *s_pmaxend;      // the regions by start, the running maximum of their ends
    int64_t nregion;
    const int32_t *winlo, *winhi;            // the read window per 256 positions
    uint64_t* keys;                          // appended; sorted into keys2 with the events' indices in vals
    IndelEvent* ev;
    int64_t cap;                             // capacity of keys and ev
    const uint64_t* keys2;
    const uint32_t* vals;
    IndelEvent* ord;                         // the events in exact order
    int64_t nev;
    himut_indel_record* recs;                // workgroup w's records start at w * 256
    uint32_t* wgcnt;
    const double *tab_hit, *tab_err;         // himut_set_indel_error_table: log10(1 - e), log10(e) per allele_class cell (null: the constant)
    unsigned long long* sc;
    int* err;
};

// a workgroup's counters: added up in LDS, one global atomic per counter and workgroup
__device__ __forceinline__ void flush_log(const uint32_t* s_log, unsigned long long* sc) {
    __syncthreads();
    if (threadIdx.x < IND_NLOG && s_log[threadIdx.x]) atomicAdd(sc + IND_SC_LOG + threadIdx.x, (unsigned long long)s_log[threadIdx.x]);
}

__device__ __forceinline__ int ref_code(const IndelArgs& A, int64_t i) {       // A T G C as 0..3 whatever the case, else -1
    return (i >= 0 && i < A.reflen) ? char2allele(upper((int)A.refseq[i])) : -1;
}

// ---- the homopolymer run behind an anchor (row 13): what the indelcal run tabulates and what a table of it is read by
constexpr int RUN_MAX = 64;                  // a longer run is "long": no class
constexpr int RUN_CLASSES = 128;             // code(b) * 32 + min(n, 32) - 1
constexpr int RUN_EVCOLS = 7;                // del1 del2 del3p ins1 ins2 ins3p other
constexpr int RUN_CELLS = RUN_CLASSES * RUN_EVCOLS;

// The run that starts at s, code_at(i) being the code of the byte at 0 <= i < reflen (A T G C as 0..3, else negative): its
// length, RUN_MAX + 1 for anything longer, and *b its letter; 0 where no run starts -- no position in front of s, the byte
// at s no letter, or the byte in front of it the same letter.  Whether a position follows the run is the caller's to ask.
template <class CodeAt>
__device__ __forceinline__ int run_at(CodeAt code_at, int64_t reflen, int64_t s, int* b) {
    if (s < 1 || s >= reflen) return 0;
    const int c = code_at(s);
    if (c < 0 || code_at(s - 1) == c) return 0;
    int n = 1;
    while (n <= RUN_MAX && s + n < reflen && code_at(s + n) == c) n++;
    *b = c;
    return n;
}
__device__ __forceinline__ int run_class(int b, int n) { return b * 32 + (n < 32 ? n : 32) - 1; }

// The column of an event against a run of n letters b: a deletion inside the run by min(L, 3), an insertion of b alone
// likewise, anything else "other".
__device__ __forceinline__ int run_event_column(int type, int L, uint64_t s0, uint64_t s1, int b, int n) {
    const int by_len = (L < 3 ? L : 3) - 1;
    if (!type) return L <= n ? by_len : 6;
    const uint64_t all_b = 0x5555555555555555ull * (uint64_t)b;
    return (s0 == (all_b & ins_keep(L)) && s1 == (all_b & ins_keep(L - 32))) ? 3 + by_len : 6;
}

// The read-independent part of an event's class: the run at a + 1 and the column, as class * RUN_EVCOLS + column, *n the
// run's length; -1 ("off run") where the byte at a + 1 is no letter, the byte at a is the same letter (the shift stopped at
// the read's start, at position 1 or at an N), or the run is long or reaches the end of the string.
__device__ __forceinline__ int allele_class(const uint8_t* refseq, int64_t reflen, int32_t a, int type, int L, uint64_t s0, uint64_t s1, int* n) {
    int b = 0;
    const int64_t s = (int64_t)a + 1;
    const int len = run_at([&](int64_t i) { return char2allele(upper((int)refseq[i])); }, reflen, s, &b);
    *n = len;
    if (len == 0 || len > RUN_MAX || !(s + len < reflen)) return -1;
    return run_class(b, len) * RUN_EVCOLS + run_event_column(type, L, s0, s1, b, len);
}

// What the first event of an allele, ord[j] = E, counts around itself: the distinct reads with the allele (run: its events),
// the distinct reads with another event at the anchor, and DP from the read window of the anchor's block.
struct AlleleTally {
    uint32_t n_alt, run, n_other, dp;
};
__device__ __forceinline__ AlleleTally allele_tally(const IndelArgs& A, const int64_t j, const IndelEvent& E) {
    const uint64_t anchor_key = E.key >> IND_KEY_SHIFT;
    uint32_t n_alt = 0, run = 0, distinct = 0, prev = 0;
    int64_t i = j;
    for (; i < A.nev; i++) {                             // the allele's run: reads ascending
        const IndelEvent B = A.ord[i];
        if (!same_allele(B, E)) break;
        if (run == 0 || B.read != prev) n_alt++;
        prev = B.read; run++;
        distinct += B.first & EV_FIRST;
    }
    for (; i < A.nev; i++) {                             // the rest of the anchor, behind and in front
        const IndelEvent B = A.ord[i];
        if ((B.key >> IND_KEY_SHIFT) != anchor_key) break;
        distinct += B.first & EV_FIRST;
    }
    for (i = j - 1; i >= 0; i--) {
        const IndelEvent B = A.ord[i];
        if ((B.key >> IND_KEY_SHIFT) != anchor_key) break;
        distinct += B.first & EV_FIRST;
    }
    const int32_t a = (int32_t)anchor_key;
    const int type = (int)((E.key >> 6) & 1u), L = (int)(E.key & 63u) + 1;
    const int32_t e_ = type ? a + 1 : a + 1 + L;
    uint32_t dp = 0;
    const int32_t rlo = A.winlo[a >> WIN_SHIFT], rhi = A.winhi[a >> WIN_SHIFT];
    for (int32_t r = rlo; r < rhi; r++) {
        const ReadMeta M = A.D.meta[r];
        if (!(M.flags & RF_SECONDARY) && !((int)A.R.mapq[r] < A.p.min_mapq) && M.tstart <= a && e_ < M.tend) dp++;
    }
    return {n_alt, run, distinct - n_alt, dp};
}

// The three-state genotype of an allele with n_alt carriers among n_non + n_alt spanning reads, per-read terms l_hit and
// l_err: fp64, no contraction, prior + n_non * x + n_alt * y in the contract's order; the state of the smallest PL (ties:
// the lower index) and the gap to the second smallest, truncated and capped at 99.
struct IndelGenotype { int state, gq; };
__device__ __forceinline__ IndelGenotype indel_genotype(const himut_indel_params& p, const uint32_t n_non, const uint32_t n_alt, const double l_hit,
                                                        const double l_err) {
    const double xs[3] = {l_hit, p.l_half, l_err}, ys[3] = {l_err, p.l_half, l_hit};
    double best = 0.0, second = 0.0;
    int state = 0;
#pragma unroll
    for (int g = 0; g < 3; g++) {
        const double t = (double)n_non * xs[g];
        const double u = (double)n_alt * ys[g];
        double sum = p.prior[g] + t;
        sum = sum + u;
        const double pl = -10.0 * sum;
        if (g == 0) { best = pl; state = 0; }
        else if (pl < best) { second = best; best = pl; state = g; }
        else if (g == 1 || pl < second) second = pl;
    }
    const double gqf = second - best;
    return {state, gqf < 99.0 ? (int)gqf : 99};
}

// An event's inserted bases as a record holds them: base i at bits 2 (i & 3) of byte i >> 2 -- the order of the 2-bit codes
// reversed.
__device__ __forceinline__ uint4 record_bases(const IndelEvent& E) {
    auto flip = [](uint64_t s) {
        const uint64_t x = __brevll(s);
        return ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    };
    const uint64_t b0 = flip(E.s0), b1 = flip(E.s1);
    return make_uint4((uint32_t)b0, (uint32_t)(b0 >> 32), (uint32_t)b1, (uint32_t)(b1 >> 32));
}

// ---- the per-event rules of the sindels run (himut_run_sindels), evaluated where an event is
// made: k_indel_events alone knows an event's raw position and query offset.  The indels and indelcal runs instantiate the
// kernel with NoRules and get the code they always had.
struct NoRules {
    static constexpr bool on = false;
};
struct SomRules {
    static constexpr bool on = true;
    const uint8_t* verdict;                  // k_sindel_reads: per read, SR_PILE | SR_PROPOSES
    int32_t min_bq, max_mismatch_count, mismatch_window_size, pad;
    double min_trim;
};
constexpr uint8_t SR_PILE = 1, SR_PROPOSES = 2;

// What one read's events need of it under SomRules (the same in the sixteen lanes of a read).
struct SomRead {
    bool proposes = false;
    int32_t qlen = 0, nm = 0;
    const int32_t* mis = nullptr;
    const uint8_t* bq = nullptr;
    double trim_start = 0.0, trim_end = 0.0;
};

// The rules on the raw event (p, q, L) of a proposing read, in the contract's order: the footprint [q - 1, qb] against the
// trim (bamlib.py:222-242, in doubles as k_dbs_propose), the read's mismatch entries in the window of (p + 1, q) minus the
// event's own, the qualities of the footprint.  The first that fails is counted; true: the event proposes.
__device__ __forceinline__ bool som_event_rules(const SomRules& S, const SomRead& rd, uint32_t* s_som, const int type, const int32_t p, const int32_t L,
                                                const int32_t q) {
    // (all three are evaluated and the first failure picked afterwards: one counter, no nest of early exits)
    const int32_t qa = q - 1, qb = type ? q + L : q;
    const bool trimmed = (double)qa < rd.trim_start || (double)qa > rd.trim_end || (double)qb < rd.trim_start || (double)qb > rd.trim_end;
    int64_t s, e;
    mismatch_range((int64_t)p + 1, q, rd.qlen, S.mismatch_window_size, s, e);
    const bool crowded = (int64_t)mismatches_in(rd.mis, rd.nm, s, e) - 1 > (int64_t)S.max_mismatch_count;
    bool low = false;
    for (int32_t x = max(qa, 0); x <= qb && x < rd.qlen; x++) low |= (int)rd.bq[x] < S.min_bq;
    const int slot = trimmed ? IND_SOM_TRIM : crowded ? IND_SOM_WINDOW : low ? IND_SOM_LOWBQ : IND_SOM_PROPOSING;
    atomicAdd(&s_som[IND_SOM_EVENTS], 1u);
    atomicAdd(&s_som[slot], 1u);
    return slot == IND_SOM_PROPOSING;
}

#ifndef HIMUT_INDELS_NO_KERNELS

// One raw event of read r over [tstart, tend): type 0 a deletion of L bases from p, type 1 L bases (query offset qsrc of
// SEQ) in front of p; q its query offset in the read (an insertion's first base, the base behind a deletion).  The rules in
// the contract's order; what survives is shifted left and staged in the workgroup's LDS: one atomic on the list's counter
// per workgroup, not per event (every event of the contig adds to that one word).
template <class Rules>
__device__ __forceinline__ void indel_event(const IndelArgs& A, const Rules& S, const SomRead& rd, uint32_t* s_log, uint32_t* s_som, IndelEvent* s_ev, uint32_t* s_n,
                                            const int64_t r, const int32_t tstart, const int32_t tend, const int type, int32_t p, const int32_t L,
                                            const int64_t qsrc, const int32_t q) {
    const int32_t e_ = type ? p : p + L;
    if (!(tstart <= p - 1 && e_ < tend) || L < 1) { atomicAdd(&s_log[IND_LOG_EDGE], 1u); return; }
    if (L > A.p.max_len) { atomicAdd(&s_log[IND_LOG_LONG], 1u); return; }
    uint64_t s0 = 0, s1 = 0;
    if (type) {
        bool bad = false;
        for (int i = 0; i < L; i++) {
            const int a = nib2allele(nib_at(A.R.seq, qsrc + i));
            if (a > 3) bad = true;
            const uint64_t b = (uint64_t)(a & 3) << (62 - 2 * (i & 31));
            if (i < 32) s0 |= b; else s1 |= b;
        }
        if (bad) { atomicAdd(&s_log[IND_LOG_NBASE], 1u); return; }
    }
    uint32_t bits = 0;                                   // what the event's last word holds beside k_indel_order's EV_FIRST
    if constexpr (Rules::on) {
        if (rd.proposes && som_event_rules(S, rd, s_som, type, p, L, q)) bits = EV_PROPOSES;
    }
    while (p - 1 > tstart) {
        const int ca = ref_code(A, (int64_t)p - 1);
        if (ca < 0) break;
        if (type) {
            if (ca != ins_base(s0, s1, L - 1)) break;
            s1 = ((s1 >> 2) | (s0 << 62)) & ins_keep(L - 32);           // the last base comes to the front
            s0 = ((s0 >> 2) | ((uint64_t)ca << 62)) & ins_keep(L);
        } else if (ca != ref_code(A, (int64_t)p + L - 1)) break;
        p--;
    }
    const int32_t a = p - 1;
    if (!in_region(A.s_start, A.s_pmaxend, A.nregion, a)) return;
    const uint64_t key = indel_key(a, type, L);
    const uint32_t k = atomicAdd(s_n, 1u);
    if (k < (uint32_t)IND_STAGE) {
        uint4* dst = reinterpret_cast<uint4*>(s_ev + k);
        dst[0] = make_uint4((uint32_t)key, (uint32_t)(key >> 32), (uint32_t)s0, (uint32_t)(s0 >> 32));
        dst[1] = make_uint4((uint32_t)s1, (uint32_t)(s1 >> 32), (uint32_t)r, bits);
        return;
    }
    // more events than the workgroup stages (reads that are mostly indels): straight to the list
    const unsigned long long slot = wave_reserve(A.sc + IND_SC_NEV);
    if ((int64_t)slot < A.cap) {
        A.keys[slot] = key;
        uint4* dst = reinterpret_cast<uint4*>(A.ev + slot);
        dst[0] = make_uint4((uint32_t)key, (uint32_t)(key >> 32), (uint32_t)s0, (uint32_t)(s0 >> 32));
        dst[1] = make_uint4((uint32_t)s1, (uint32_t)(s1 >> 32), (uint32_t)r, bits);
    }
}

template <class Rules>
__global__ void __launch_bounds__(256) k_indel_events(IndelArgs A, Rules S) {
    __shared__ __align__(16) IndelEvent s_ev[IND_STAGE];
    __shared__ uint32_t s_log[16];
    __shared__ uint32_t s_som[8];
    __shared__ uint32_t s_n;
    __shared__ unsigned long long s_base;
    if (threadIdx.x < 16) s_log[threadIdx.x] = 0;
    if constexpr (Rules::on) {
        if (threadIdx.x < 8) s_som[threadIdx.x] = 0;
    }
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int gl = threadIdx.x & 15;
    if (r < A.R.n && !*A.err) {
        const ReadMeta M = A.D.meta[r];
        if (!(M.flags & RF_SECONDARY) && !((int)A.R.mapq[r] < A.p.min_mapq)) {
            const Seg* segs = A.D.segs + M.segbase;
            const int32_t qstart = A.R.qstart[r];
            SomRead rd;
            if constexpr (Rules::on) {
                rd.proposes = (S.verdict[r] & SR_PROPOSES) != 0;
                if (rd.proposes) {
                    rd.qlen = A.R.qlen[r]; rd.nm = A.D.nmis[r];
                    rd.mis = A.D.mis + M.segbase; rd.bq = A.R.bq + M.qoff;
                    rd.trim_start = floor(S.min_trim * (double)rd.qlen);               // bamlib.py:226
                    rd.trim_end = ceil((1.0 - S.min_trim) * (double)rd.qlen);          // bamlib.py:227
                }
            }
            for (int j = gl; j < M.nseg; j += 16) {
                const Seg g = segs[j];
                if constexpr (Rules::on) {                   // one call site for both kinds: the rules make the inlined body large
#pragma unroll 1
                    for (int t = 1; t >= 0; t--) {
                        if (!(g.flags & (t ? SEG_INS : SEG_DEL))) continue;
                        int32_t L = g.len, q = g.q0;
                        if (t) {
                            q = qstart;
                            if (j > 0) { const Seg b = segs[j - 1]; q = b.q0 + ((b.flags & SEG_DEL) ? 0 : b.len); }
                            L = g.q0 - q;
                        }
                        indel_event(A, S, rd, s_log, s_som, s_ev, &s_n, r, M.tstart, M.tend, t, g.t0, L, M.qoff + q, q);
                    }
                    continue;
                }
                if (g.flags & SEG_INS) {                     // (in front of a deletion too: "+ac-gt")
                    int32_t qend = qstart;                   // the query offset behind the previous segment
                    if (j > 0) { const Seg b = segs[j - 1]; qend = b.q0 + ((b.flags & SEG_DEL) ? 0 : b.len); }
                    indel_event(A, S, rd, s_log, s_som, s_ev, &s_n, r, M.tstart, M.tend, 1, g.t0, g.q0 - qend, M.qoff + qend, qend);
                }
                if (g.flags & SEG_DEL) indel_event(A, S, rd, s_log, s_som, s_ev, &s_n, r, M.tstart, M.tend, 0, g.t0, g.len, 0, g.q0);
            }
        }
    }
    __syncthreads();
    // ---- the staged events behind one another in the list
    const uint32_t staged = min(s_n, (uint32_t)IND_STAGE);
    if (threadIdx.x == 0 && staged) s_base = atomicAdd(A.sc + IND_SC_NEV, (unsigned long long)staged);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < staged; k += 256) {
        const int64_t slot = (int64_t)s_base + k;
        if (slot < A.cap) {
            const uint4* src = reinterpret_cast<const uint4*>(s_ev + k);
            uint4* dst = reinterpret_cast<uint4*>(A.ev + slot);
            const uint4 lo = src[0];
            A.keys[slot] = (uint64_t)lo.x | ((uint64_t)lo.y << 32);
            dst[0] = lo; dst[1] = src[1];
        }
    }
    flush_log(s_log, A.sc);
    if constexpr (Rules::on) {
        if (threadIdx.x < IND_NSOM && s_som[threadIdx.x]) atomicAdd(A.sc + IND_SC_SOM + threadIdx.x, (unsigned long long)s_som[threadIdx.x]);
    }
}

// The place of sorted event j among the events of its key (the same anchor, type and length) by (bases, read); equal
// ones -- a read that yields an allele twice -- keep the order the sort left them in.  Groups are as small as the pile is
// deep: every thread counts through its own.
__global__ void __launch_bounds__(256) k_indel_order(IndelArgs A) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= A.nev) return;
    const uint64_t key = A.keys2[j];
    IndelEvent E = A.ev[A.vals[j]];
    int64_t g0 = j, rank = 0;
    bool in_key = true;
    uint32_t first = 1;
    for (int64_t i = j - 1; i >= 0; i--) {
        const uint64_t k = A.keys2[i];
        if ((k >> IND_KEY_SHIFT) != (key >> IND_KEY_SHIFT)) break;
        if (k != key) in_key = false;
        const IndelEvent B = A.ev[A.vals[i]];
        if (B.read == E.read) first = 0;
        if (in_key) { g0 = i; if (!event_less(E, B)) rank++; }
        else if (!first) break;
    }
    for (int64_t i = j + 1; i < A.nev && A.keys2[i] == key; i++)
        if (event_less(A.ev[A.vals[i]], E)) rank++;
    E.first = (E.first & EV_PROPOSES) | first;
    A.ord[g0 + rank] = E;
}

__global__ void __launch_bounds__(256) k_indel_eval(IndelArgs A) {
    __shared__ uint32_t s_log[16];
    __shared__ int s_e[4];
    const int tid = threadIdx.x;
    if (tid < 16) s_log[tid] = 0;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + tid;
    bool emit = false;
    uint4 w0 = make_uint4(0, 0, 0, 0), w1 = w0, w2 = w0;
    if (j < A.nev && !*A.err) {
        const IndelEvent E = A.ord[j];
        if (j == 0 || !same_allele(A.ord[j - 1], E)) {           // the first of its allele
            const AlleleTally T = allele_tally(A, j, E);
            const uint32_t n_alt = T.n_alt, run = T.run, n_other = T.n_other, dp = T.dp;
            const int32_t a = (int32_t)(E.key >> IND_KEY_SHIFT);
            const int type = (int)((E.key >> 6) & 1u), L = (int)(E.key & 63u) + 1;
            const uint32_t n_non = dp - n_alt;
            // the per-read terms: the constant, or under a table (himut_set_indel_error_table) the allele's cell of it
            double l_hit = A.p.l_hit, l_err = A.p.l_err;
            if (A.tab_hit) {
                int n_run;
                const int cell = allele_class(A.refseq, A.reflen, a, type, L, E.s0, E.s1, &n_run);
                if (cell >= 0) { l_hit = A.tab_hit[cell]; l_err = A.tab_err[cell]; }
            }
            const IndelGenotype G = indel_genotype(A.p, n_non, n_alt, l_hit, l_err);
            const int state = G.state, gq = G.gq;
            atomicAdd(&s_log[IND_LOG_ALLELES], 1u);
            if (run > n_alt) atomicAdd(&s_log[IND_LOG_DUP], run - n_alt);
            atomicAdd(&s_log[IND_LOG_STATE + state], 1u);
            int status = HIMUT_ST_PASS;
            if (state != 0) {
                int slot = IND_LOG_PASS;
                if (gq < A.p.min_gq) { status = HIMUT_ST_LOWGQ; slot = IND_LOG_LOWGQ; }
                else if ((int64_t)n_alt < A.p.min_alt_count || (state == 1 && (int64_t)n_non < A.p.min_ref_count)) { status = HIMUT_ST_LOWDEPTH; slot = IND_LOG_LOWDEPTH; }
                else if ((int64_t)dp > A.p.md_threshold) { status = HIMUT_ST_HIGHDEPTH; slot = IND_LOG_HIGHDEPTH; }
                atomicAdd(&s_log[slot], 1u);
            }
            if (state != 0 || A.p.report_homref) {
                emit = true;
                w0 = make_uint4((uint32_t)a, (uint32_t)L, (uint32_t)type | ((uint32_t)status << 8) | ((uint32_t)state << 16), (uint32_t)gq);
                w1 = make_uint4(dp, n_alt, n_other, 0u);
                w2 = record_bases(E);
            }
        }
    }
    // ---- the workgroup's records in thread (= allele) order
    const WgRank e = wg_rank<4>(emit, s_e);
    if (emit) {
        uint4* dst = reinterpret_cast<uint4*>(A.recs + ((int64_t)blockIdx.x * 256 + e.rank));
        dst[0] = w0; dst[1] = w1; dst[2] = w2; dst[3] = make_uint4(0, 0, 0, 0);
    }
    if (tid == 0) A.wgcnt[blockIdx.x] = (uint32_t)e.total;
    flush_log(s_log, A.sc);
}

#endif  // HIMUT_INDELS_NO_KERNELS

// ---- host side (himut_indels.hip): the front the indels and indelcal runs share, on an event list L of the run's own.
//   indel_front_check  what a run needs before it starts: max_len in 1..64, reads, regions, the reference string, no
//                      region with start > end (who: the caller's name, for the message)
//   indel_front_run    EV_START .. EV_GATHER: the region tables, the cs decode under open gates, the read windows, the
//                      events (k_indel_events), their sort and exact order (k_indel_order).  L.d_sc holds the decode's
//                      Scalars, the IND_SC_WORDS words and `own_words` more for the caller, all cleared behind EV_START;
//                      reserve_more(c, cap) sizes what else of the caller's depends on the event capacity.  allow_spec:
//                      on the capacity L keeps; F->over then says that the events did not fit (run_repeating).
struct IndelFront {
    IndelArgs A;                             // everything up to ord and nev filled in
    Scalars* sc;
    unsigned long long* words;               // the IND_SC_WORDS words; the caller's own follow
    int64_t nev, cap, nblk, nreg, positions;
    bool spec, over;
};
//                      som (the sindels run alone): the identity threshold the decode runs under -- nothing else of its
//                      parameter block differs, so the pile and the events are the ones of the open gate --, read_pass,
//                      queued between the decode and the events (it leaves rules.verdict), and the rules
//                      k_indel_events<SomRules> applies.
struct IndelSomatic {
    double min_sequence_identity;
    int32_t min_qv, qlen_lower_limit, qlen_upper_limit;    // the rest of call's read filters, for read_pass
    SomRules rules;
    void (*read_pass)(himut_ctx*, const IndelArgs&, const IndelSomatic&);
};
int indel_front_check(himut_ctx* c, int32_t max_len, const char* who);
void indel_front_run(himut_ctx* c, IndelEventList& L, const himut_indel_params& p, bool allow_spec, size_t own_words,
                     void (*reserve_more)(himut_ctx*, int64_t cap), IndelFront* F, const IndelSomatic* som = nullptr);

}  // namespace himut
