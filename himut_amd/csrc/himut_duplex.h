// The kernels of himut_run_duplex (himut_duplex.hip): the substitutions that both reads of a molecule show, the ones only
// one of them shows, and the positions at which both could have shown one.  The contract is include/himut_hip.h
// (himut_run_duplex) and DESIGN.md section 8, row 19.
//
//   k_duplex_reads         a wave per read: the read's qualities once (wave_bq_sum) and call's read filters as one byte per
//                          read, DV_PROPOSES or the first cause it fails (the front has had no capture yet, which is where
//                          the other runs get the quality sums from)
//   k_duplex_events<false> sixteen lanes per read of a pair in play, a lane per substitution of its mismatch list in turns
//                          of sixteen: the read's own rules, the mate's state at the position (a search of the mate's
//                          segments), the counters, the single-strand spectrum, and from the read with the lower index a
//                          key per double-strand event inside a chunk
//   k_duplex_overlap       the denominator, a wave per pair in play: the positions of the two reads' overlap in turns of
//                          256, both query offsets from the segment lists (kept in scalar registers while a turn stays
//                          inside one segment, the lanes' own searches where it does not), a quality byte of either read
//                          per lane and position
//   k_duplex_sites         a thread per distinct key (the sorted keys run-length encoded: the run's length is n_ds): the
//                          position and the allele code the sites pass takes
//   k_duplex_events<true>  the same walk over every pile read's substitutions, against the distinct keys: n_ss, n_alt_unpaired
//   k_duplex_records       a thread per candidate: the sites pass's record with the three counts behind it
//
// The genotype and the verdict of a candidate are the sites run's kernels (sites_back, himut_sites.hip).
#pragma once

#include "himut_device.h"

namespace himut {

static_assert(sizeof(himut_duplex_params) == 32, "himut_duplex_params is 32 bytes (DuplexParams of _ffi.py)");
static_assert(sizeof(himut_duplex_record) == 80 && offsetof(himut_duplex_record, site) == 0 && offsetof(himut_duplex_record, n_ds) == 64 &&
              offsetof(himut_duplex_record, n_ss) == 68 && offsetof(himut_duplex_record, n_alt_unpaired) == 72,
              "himut_duplex_record: the site record, then the three counts (DUPLEX_RECORD_DTYPE of _ffi.py)");

// a read's verdict: it proposes, or the first cause it does not (the order of himut_get_duplex's pairs_* counters)
enum : uint8_t { DV_PROPOSES = 0, DV_NOTPILE = 1, DV_IDENTITY = 2, DV_LOWQV = 3, DV_QLEN = 4 };
// the mate's state at an event's position, in the order of the counters; DM_UNHELD: spanned, but no segment holds it
enum : int { DM_NOCOVER = 0, DM_DEL, DM_LOWBQ, DM_TRIM, DM_CONCORDANT, DM_SINGLE, DM_OTHER, DM_UNHELD };

// the run's scalars (unsigned long long each).  The first DX_ONCE_WORDS are written once per run; the rest by
// k_duplex_events<false>, which the host may launch twice (count_keys) and clears in front of each launch.
constexpr int DX_W_READS = 0, DX_W_PILE = 1, DX_W_PROPOSING = 2, DX_W_DSBASES = 3, DX_W_OVERLAP = 4, DX_ONCE_WORDS = 8;
constexpr int DX_W_NCAND = 5;                                                       // the distinct keys (the run-length encoding's count)
constexpr int DX_W_PAIRS = 8, DX_W_INPLAY = 9, DX_W_CAUSE = 10;                     // 10..13: not pile, identity, quality sum, query length
constexpr int DX_W_EVENTS = 14, DX_W_OWN = 15;                                      // 15..17: num_trim, num_window, num_lowbq
constexpr int DX_W_STATE = 18;                                                      // 18..24: DM_NOCOVER .. DM_OTHER
constexpr int DX_W_MATEWIN = 25, DX_W_DS = 26, DX_W_NKEYS = 27, DX_W_SS = 28;       // 28..39: ss[12]
constexpr int DX_WORDS = 40;
constexpr int DX_WG_WORDS = DX_WORDS - DX_ONCE_WORDS;
constexpr int DX_STAGE = 1024;                                                      // keys a workgroup of the events kernel stages in LDS                               // what a workgroup of the events kernel adds up in LDS

struct DuplexArgs {
    Reads R;
    Derived D;
    himut_params p;              // call's thresholds (himut_set_params)
    const int32_t* mate;         // checked by the host: -1, or another read whose mate is this one
    uint8_t* verdict;            // DV_* per read
    const int32_t *s_start, *s_pmaxend;      // the chunks by start, the running maximum of their ends
    int64_t nregion;
    uint64_t* keys;              // k_duplex_events<false>: a key per double-strand event inside a chunk, none past cap_keys
    int64_t cap_keys;
    const uint64_t* uniq;        // k_duplex_events<true>: the distinct keys ascending
    int64_t ncand;
    uint32_t* tally;             // ... and per key {n_ss, n_alt_unpaired}
    unsigned long long* w;       // DX_WORDS words
    int* err;
};

// tpos << 4 | ref << 2 | alt: ascending keys = ascending (tpos, ref, alt), alleles A0 T1 G2 C3; code is an mq[] entry's low
// four bits
__device__ __forceinline__ uint64_t duplex_key(int32_t tpos, uint32_t code) { return ((uint64_t)(uint32_t)tpos << 4) | (uint64_t)(code & 15u); }

// start <= p < end for some chunk
__device__ __forceinline__ bool in_chunk(const DuplexArgs& A, int32_t p) {
    const int64_t k = upper_bound(A.s_start, (int64_t)0, A.nregion, p);
    return k > 0 && A.s_pmaxend[k - 1] > p;
}

// what the look-ups of one lane need of a read
struct DuplexRead {
    const Seg* segs;
    const int32_t* mis;
    int64_t qo;
    int32_t ns, nm, tstart, tend, qlen;
    double trim_start, trim_end;
};

__device__ __forceinline__ DuplexRead duplex_read(const DuplexArgs& A, int64_t r) {
    const ReadMeta M = A.D.meta[r];
    DuplexRead X;
    X.segs = A.D.segs + M.segbase; X.mis = A.D.mis + M.segbase; X.qo = M.qoff;
    X.ns = M.nseg; X.nm = A.D.nmis[r]; X.tstart = M.tstart; X.tend = M.tend; X.qlen = A.R.qlen[r];
    X.trim_start = floor(A.p.min_trim * (double)X.qlen);               // bamlib.py:226
    X.trim_end = ceil((1.0 - A.p.min_trim) * (double)X.qlen);          // bamlib.py:227
    return X;
}

__device__ __forceinline__ bool duplex_trimmed(const DuplexRead& X, int32_t q) { return (double)q < X.trim_start || (double)q > X.trim_end; }

// the read's mismatch entries in the window of (tpos, q), minus the one at tpos itself, exceed max_mismatch_count
__device__ __forceinline__ bool duplex_crowded(const DuplexArgs& A, const DuplexRead& X, int32_t tpos, int32_t q) {
    int64_t s, e;
    mismatch_range((int64_t)tpos, q, X.qlen, A.p.mismatch_window_size, s, e);
    return (int64_t)mismatches_in(X.mis, X.nm, s, e) - 1 > (int64_t)A.p.max_mismatch_count;
}

// The first segment of X from `from` on that ends behind rpos (segments are in order and do not overlap): its index, X.ns
// for none.
__device__ __forceinline__ int duplex_seg(const DuplexRead& X, int from, int32_t rpos) {
    int lo = from, hi = X.ns;
    while (lo < hi) { const int m = (lo + hi) >> 1; if (rpos >= X.segs[m].t0 + X.segs[m].len) lo = m + 1; else hi = m; }
    return lo;
}

// What X holds at rpos, tstart <= rpos < tend: DM_UNHELD, DM_DEL, DM_LOWBQ, DM_TRIM, or DM_OTHER for an aligned base of
// quality >= min_bq outside the trimmed ends, with *q its query offset; *seg: duplex_seg's answer.
__device__ __forceinline__ int duplex_base(const DuplexArgs& A, const DuplexRead& X, int from, int32_t rpos, int32_t* q, int* seg) {
    const int j = *seg = duplex_seg(X, from, rpos);
    if (j >= X.ns) return DM_UNHELD;
    const Seg sg = X.segs[j];
    if (rpos < sg.t0) return DM_UNHELD;
    if (sg.flags & SEG_DEL) return DM_DEL;
    *q = sg.q0 + (rpos - sg.t0);
    if ((int32_t)A.R.bq[X.qo + *q] < A.p.min_bq) return DM_LOWBQ;
    if (duplex_trimmed(X, *q)) return DM_TRIM;
    return DM_OTHER;
}

// the mate B's state at rpos against (ref, alt) in allele indices; *q: B's query offset where it holds a base
__device__ __forceinline__ int duplex_mate_state(const DuplexArgs& A, const DuplexRead& B, int32_t rpos, int ref, int alt, int32_t* q) {
    if (!(B.tstart <= rpos && rpos < B.tend)) return DM_NOCOVER;
    int seg;
    const int st = duplex_base(A, B, 0, rpos, q, &seg);
    if (st != DM_OTHER) return st;
    const int b = nib2allele(nib_at(A.R.seq, B.qo + *q));
    return b == alt ? DM_CONCORDANT : b == ref ? DM_SINGLE : DM_OTHER;
}

struct DuplexReadArgs {
    Reads R;
    const ReadMeta* meta;
    int32_t min_mapq, min_qv, qlen_lower_limit, qlen_upper_limit;
    uint8_t* verdict;
    unsigned long long* w;
    const int* err;
};

__global__ void __launch_bounds__(256) k_duplex_reads(DuplexReadArgs A) {
    __shared__ uint32_t s_cnt[3];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + uni((int)(threadIdx.x >> 6));
    if (r < A.R.n && !*A.err) {
        const uint32_t flags = uni(A.meta[r].flags);
        const int mapq = uni((int)A.R.mapq[r]);
        uint8_t verdict = DV_NOTPILE;
        if (!(flags & RF_SECONDARY) && !(mapq < A.min_mapq)) {
            const int32_t qlen = max(uni(A.R.qlen[r]), 0);
            const uint64_t sum = wave_bq_sum(A.R.bq + uni(A.R.qoff[r]), qlen, lane);
            // call's read filters (caller.py:310-317), as k_sindel_reads applies them
            verdict = !(flags & RF_IDENT_OK) ? DV_IDENTITY : sum < (uint64_t)(int64_t)max(A.min_qv, 0) * (uint64_t)(uint32_t)qlen ? DV_LOWQV :
                      !(A.qlen_lower_limit < qlen && qlen < A.qlen_upper_limit) ? DV_QLEN : DV_PROPOSES;
        }
        if (lane == 0) {
            A.verdict[r] = verdict;
            atomicAdd(&s_cnt[DX_W_READS], 1u);
            if (verdict != DV_NOTPILE) atomicAdd(&s_cnt[DX_W_PILE], 1u);
            if (verdict == DV_PROPOSES) atomicAdd(&s_cnt[DX_W_PROPOSING], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(A.w + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

// the class of ref > alt (allele indices) among A>C A>G A>T C>A .. T>G, on the strand of a read with SAM flag `flag`
__device__ __forceinline__ int duplex_ss_class(int ref, int alt, uint32_t flag) {
    if (flag & 0x10u) { ref ^= 1; alt ^= 1; }                       // A0 <-> T1, G2 <-> C3
    const int a = asc_rank(ref), b = asc_rank(alt);
    return a * 3 + b - (b > a ? 1 : 0);
}

template <bool TALLY>
__global__ void __launch_bounds__(256) k_duplex_events(DuplexArgs A) {
    __shared__ uint32_t s_cnt[DX_WG_WORDS];
    __shared__ uint64_t s_keys[TALLY ? 1 : DX_STAGE];                // the workgroup's keys: one atomic on the list's counter per
    __shared__ uint32_t s_nkeys;                                     // workgroup, not per key (every key of the contig adds to it)
    __shared__ unsigned long long s_base;
    if (threadIdx.x < DX_WG_WORDS) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_nkeys = 0;
    __syncthreads();
    auto count = [&](int word) { if (!TALLY) atomicAdd(&s_cnt[word - DX_ONCE_WORDS], 1u); };
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int gl = threadIdx.x & 15;
    if (r < A.R.n && !*A.err) {
        const int32_t m = A.mate[r];
        const uint8_t vr = A.verdict[r], vm = m >= 0 ? A.verdict[m] : (uint8_t)DV_NOTPILE;
        const bool play = m >= 0 && vr == DV_PROPOSES && vm == DV_PROPOSES;
        if (gl == 0 && (int64_t)m > r) {                             // a pair is counted by its lower read
            count(DX_W_PAIRS);
            const int cause = vr == DV_PROPOSES ? (int)vm : vm == DV_PROPOSES ? (int)vr : min((int)vr, (int)vm);
            count(play ? DX_W_INPLAY : DX_W_CAUSE + cause - 1);
        }
        if (TALLY ? vr != DV_NOTPILE : play) {
            const DuplexRead X = duplex_read(A, r);
            DuplexRead B = X;
            if (play) B = duplex_read(A, m);
            const uint32_t* mq = A.D.mq + (X.mis - A.D.mis);
            const uint32_t flag = A.R.flag[r];
            for (int e = gl; e < X.nm; e += 16) {
                const uint32_t v = mq[e];
                if (!(v & 16u)) continue;                            // an insertion or a deletion
                const int32_t tpos = X.mis[e], qa = (int32_t)(v >> 5);
                const int ref = (int)(v >> 2) & 3, alt = (int)v & 3;
                const uint64_t key = duplex_key(tpos, v);
                int64_t j = 0;
                if (TALLY) {
                    j = lower_bound(A.uniq, (int64_t)0, A.ncand, key);
                    if (j >= A.ncand || A.uniq[j] != key) continue;
                    if (!play) { atomicAdd(A.tally + 2 * j + 1, 1u); continue; }
                }
                // the read's own rules: all three evaluated, the first failure picked (som_event_rules, himut_indels.h)
                const bool trimmed = duplex_trimmed(X, qa), crowded = duplex_crowded(A, X, tpos, qa);
                const bool low = (int32_t)A.R.bq[X.qo + qa] < A.p.min_bq;
                count(DX_W_EVENTS);
                if (trimmed || crowded || low) { count(DX_W_OWN + (trimmed ? 0 : crowded ? 1 : 2)); continue; }
                int32_t qb = 0;
                const int st = duplex_mate_state(A, B, tpos - 1, ref, alt, &qb);
                if (st == DM_UNHELD) { set_err(A.err, HIMUT_ERR_COVER); continue; }
                if (TALLY) { if (st == DM_SINGLE) atomicAdd(A.tally + 2 * j, 1u); continue; }
                count(DX_W_STATE + st);
                const bool inside = in_chunk(A, tpos - 1);
                if (st == DM_SINGLE && inside) count(DX_W_SS + duplex_ss_class(ref, alt, flag));
                if (st != DM_CONCORDANT) continue;
                if (duplex_crowded(A, B, tpos, qb)) { count(DX_W_MATEWIN); continue; }
                if (r > (int64_t)m) continue;                        // the mate counts the event
                count(DX_W_DS);
                if (!inside) continue;
                const uint32_t k = atomicAdd(&s_nkeys, 1u);
                if (k < (uint32_t)DX_STAGE) { s_keys[k] = key; continue; }
                // more keys than the workgroup stages: straight to the list
                const unsigned long long slot = atomicAdd(A.w + DX_W_NKEYS, 1ull);
                if ((int64_t)slot < A.cap_keys) A.keys[slot] = key;
            }
        }
    }
    if (TALLY) return;
    __syncthreads();
    const uint32_t staged = min(s_nkeys, (uint32_t)DX_STAGE);
    if (threadIdx.x == 0 && staged) s_base = atomicAdd(A.w + DX_W_NKEYS, (unsigned long long)staged);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < staged; k += 256)
        if ((int64_t)(s_base + k) < A.cap_keys) A.keys[s_base + k] = s_keys[k];
    if (threadIdx.x < DX_WG_WORDS && s_cnt[threadIdx.x]) atomicAdd(A.w + DX_ONCE_WORDS + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

// A read's segment under a run of 64 positions, kept in scalar registers while the run stays inside it.
struct DuplexSpan {
    int j;                       // the segment's index (X.ns: none)
    int32_t t0, t1, q0;
    uint32_t flags;
};
__device__ __forceinline__ DuplexSpan duplex_span(const DuplexRead& X, int j) {
    DuplexSpan S{j, 0, 0, 0, 0u};
    if (j < X.ns) {
        const Seg g = X.segs[j];
        S.t0 = uni(g.t0); S.t1 = uni(g.t0 + g.len); S.q0 = uni(g.q0); S.flags = uni(g.flags);
    }
    return S;
}

// What the chunks say of the positions from p on, for a wave: *inside, and the first position behind p it does not hold
// for (in_chunk's search, once per stretch instead of once per lane and position).
__device__ __forceinline__ int64_t duplex_chunk_stretch(const DuplexArgs& A, int32_t p, bool* inside) {
    const int64_t k = upper_bound(A.s_start, (int64_t)0, A.nregion, p);
    *inside = k > 0 && A.s_pmaxend[k - 1] > p;
    if (*inside) return (int64_t)A.s_pmaxend[k - 1];                 // the chunk with that end starts at or in front of p
    return k < A.nregion ? (int64_t)A.s_start[k] : (int64_t)INT32_MAX + 1;
}

// The positions of the overlap in turns of DX_TURN, a lane at every 64th.  A turn that lies inside one segment of either
// read and on one side of the chunks' edges costs two quality bytes a lane and position and nothing else, the loads of
// its four positions in flight together; a turn that crosses a segment's end or a chunk's edge takes the lanes' own
// searches (duplex_base, in_chunk) and then finds the segments its last position lies in.
constexpr int DX_TURN = 256;

__global__ void __launch_bounds__(256) k_duplex_overlap(DuplexArgs A) {
    __shared__ uint32_t s_cnt[2];
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + uni((int)(threadIdx.x >> 6));
    if (r < A.R.n && !*A.err) {
        const int32_t m = uni(A.mate[r]);
        if ((int64_t)m > r && A.verdict[r] == DV_PROPOSES && A.verdict[m] == DV_PROPOSES) {
            const DuplexRead X = duplex_read(A, r), B = duplex_read(A, m);
            const int64_t lo = uni((int64_t)max(X.tstart, B.tstart)), hi = uni((int64_t)min(X.tend, B.tend));
            int mine = 0;                                            // this lane's positions
            bool unheld = false;
            if (lo < hi) {
                DuplexSpan sa = duplex_span(X, uni(duplex_seg(X, 0, (int32_t)lo))), sb = duplex_span(B, uni(duplex_seg(B, 0, (int32_t)lo)));
                bool inside = false;
                int64_t until = lo;                                  // the chunks' answer `inside` holds in front of `until`
                for (int64_t p0 = lo; p0 < hi; p0 += DX_TURN) {
                    const int64_t last = min(p0 + DX_TURN - 1, hi - 1);
                    if (p0 >= until) until = uni(duplex_chunk_stretch(A, (int32_t)p0, &inside));
                    const bool one_side = last < until;
                    const bool in_a = sa.j < X.ns && sa.t0 <= p0 && last < sa.t1, in_b = sb.j < B.ns && sb.t0 <= p0 && last < sb.t1;
                    if (in_a && in_b && one_side) {
                        if (!inside || ((sa.flags | sb.flags) & SEG_DEL)) continue;
                        int32_t qa[DX_TURN / 64], qb[DX_TURN / 64];
                        int32_t ba[DX_TURN / 64], bb[DX_TURN / 64];  // the qualities; -1 behind the turn's last position
#pragma unroll
                        for (int k = 0; k < DX_TURN / 64; k++) {
                            const int64_t p = p0 + 64 * k + lane;
                            qa[k] = sa.q0 + (int32_t)(p - sa.t0); qb[k] = sb.q0 + (int32_t)(p - sb.t0);
                            ba[k] = p <= last ? (int32_t)A.R.bq[X.qo + qa[k]] : -1;
                            bb[k] = p <= last ? (int32_t)A.R.bq[B.qo + qb[k]] : -1;
                        }
#pragma unroll
                        for (int k = 0; k < DX_TURN / 64; k++)
                            mine += (ba[k] >= 0 && ba[k] >= A.p.min_bq && bb[k] >= A.p.min_bq && !duplex_trimmed(X, qa[k]) && !duplex_trimmed(B, qb[k])) ? 1 : 0;
                    } else {
                        for (int k = 0; k < DX_TURN / 64; k++) {
                            const int64_t p = p0 + 64 * k + lane;
                            if (p > last) continue;
                            int32_t qa = 0, qb = 0;
                            int ia, ib;
                            const int ua = duplex_base(A, X, sa.j, (int32_t)p, &qa, &ia), ub = duplex_base(A, B, sb.j, (int32_t)p, &qb, &ib);
                            unheld |= ua == DM_UNHELD || ub == DM_UNHELD;
                            mine += (ua == DM_OTHER && ub == DM_OTHER && (one_side ? inside : in_chunk(A, (int32_t)p))) ? 1 : 0;
                        }
                        sa = duplex_span(X, uni(duplex_seg(X, sa.j, (int32_t)last))); sb = duplex_span(B, uni(duplex_seg(B, sb.j, (int32_t)last)));
                    }
                }
            }
            const uint32_t n = (uint32_t)lane_val(wave_incl_add(mine, lane), 63);
            unheld = __ballot(unheld) != 0;
            if (unheld) set_err(A.err, HIMUT_ERR_COVER);
            if (lane == 0 && n) { atomicAdd(&s_cnt[0], n); atomicAdd(&s_cnt[1], 1u); }
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(A.w + DX_W_DSBASES + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

// the distinct keys as the sites pass's arrays
__global__ void __launch_bounds__(256) k_duplex_sites(const uint64_t* uniq, int64_t n, int32_t* pos1, uint8_t* code) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    pos1[j] = (int32_t)(uniq[j] >> 4);
    code[j] = (uint8_t)(uniq[j] & 15u);
}

__global__ void __launch_bounds__(256) k_duplex_records(const himut_site_record* site, const uint32_t* n_ds, const uint32_t* tally, int64_t n,
                                                        himut_duplex_record* out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint4* src = reinterpret_cast<const uint4*>(site + j);
    uint4* dst = reinterpret_cast<uint4*>(out + j);
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
    dst[4] = make_uint4(n_ds[j], tally[2 * j], tally[2 * j + 1], 0u);
}

}  // namespace himut
