// Device code of the normcounts sweep: himut's `normcounts.get_callable_tricounts`
// (src/himut/normcounts.py:206-421, with or without --phase) on the machinery of the call path.
//
// Every reference position of the chunks is genotyped from its pile column and, when callable, binned by
// trinucleotide context.  A pile cell is the 16-bit value of the call path (CELL_* code, CELL_INS, BQ) with one
// more bit: "this base counts as callable for its read" (update_tri2count, normcounts.py:66-110).
//
//   k_read_live    sixteen lanes per read: the read filters but the mean quality (normcounts.py:302-309), cs-vs-SEQ check
//   k_callable     wave per read: one bit per query base (the mismatch-window / trim / BQ rules); the mean-quality filter
//                  (it reads every quality anyway), num_ccs
//   k_norm_plan, k_norm_quad (himut_normq.h)
//                  the sweep in use: per 256 positions the list of the reads' gapless pieces over them, then a wave per 256
//                  positions, four columns per lane, no cells in memory; classifies the columns that hold nothing but the
//                  reference allele, lists the others
//   k_norm_dirty   lane per listed position: the general classification (ten PLs twice, PoN / common look-ups)
//   k_norm_tile    round 2's first sweep: workgroup per 256-position tile of a chunk, the cells of the reads over the tile
//                  built in LDS, 48 rows at a time, every thread down its column.  It takes the tiles k_norm_quad leaves
//                  alone (from a list) and the whole contig when a list was too short.
//
// The arguments (NormArgs), the tile sweep itself and the classification of a position (norm_classify, norm_tally), which
// k_norm_tile, k_norm_dirty and the callable run's k_callmap_sweep (himut_callmap.h) all call, are himut_sweep.h's.
#pragma once

#include "himut_sweep.h"

namespace himut {

// ---------------------------------------------------------------------------------------
// phased runs: a read counts in a chunk only if it carries haplotype 0 or 1 there (normcounts.py:293-298)
__global__ void __launch_bounds__(256) k_pair_ccs(Chunks C, Phase H, Reads R, const uint8_t* live, int64_t npairs,
                                                  uint8_t* ccs_flag) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= npairs) return;
    const int64_t c = upper_bound(C.pairoff, (int64_t)0, C.n + 1, k) - 1;
    const int64_t r = C.rlo[c] + (k - C.pairoff[c]);
    if (live[r] && H.hap[k] != HAP_NONE) ccs_flag[R.qid[r]] = 1;
}

__global__ void __launch_bounds__(256) k_read_live(Reads R, Derived D, Chunks C, Params P, uint8_t* live, uint8_t* ccs_flag,
                                                   int* err) {
    // sixteen lanes per read: the substitution check runs down the mismatch list sixteen entries at a time (a noisy
    // read has hundreds); the rest is lane 0 of the group
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int gl = threadIdx.x & 15;
    if (r >= R.n) return;
    const ReadMeta M = D.meta[r];
    uint8_t lv = 0;
    if (!(M.flags & RF_SECONDARY)) {
        // substitutions: the base cs names must be the base SEQ holds (the pile takes it from SEQ)
        const int nm = D.nmis[r];
        const uint32_t* mq = D.mq + M.segbase;
        int bad = 0;
        for (int e = gl; e < nm; e += 16) {
            const uint32_t v = mq[e];
            if (v & 16u) {
                const int qa = nib2allele(nib_at(R.seq, M.qoff + (v >> 5)));
                if (qa > 3) bad = HIMUT_ERR_BASE;
                else if (qa != (int)(v & 3u)) bad = HIMUT_ERR_CS;
            }
        }
        if (bad) set_err(err, bad);
        // a read with a base outside ATGC somewhere (k_flag_bases): KeyError in the reference's pile if the base is aligned
        // and some chunk fetches the read (normcounts.py:289,117; every fetched read is piled, whatever its filters say)
        if (R.nonacgt && R.nonacgt[r] && M.nseg > 0) {
            int64_t lo = 0, hi = C.n;
            while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (C.rec[m].start < M.tend) lo = m + 1; else hi = m; }
            if (lo > 0 && C.rec[lo - 1].pmaxend > M.tstart && !aligned_bases_ok(R, D.segs + M.segbase, M.nseg, M.qoff, gl, 16))
                set_err(err, HIMUT_ERR_BASE);
        }
        if (gl != 0) return;
        const int32_t qlen = R.qlen[r];
        bool ok = (M.flags & RF_IDENT_OK) != 0;
        // (the mean quality, the last of the read filters, is k_callable's: it is the kernel that reads every quality)
        if ((int)R.mapq[r] < P.p.min_mapq) ok = false;
        if (!(P.p.qlen_lower_limit < qlen && qlen < P.p.qlen_upper_limit)) ok = false;
        if (ok) {
            // fetched by some chunk: start < tend and end > tstart (normcounts.py:289)
            int64_t lo = 0, hi = C.n;
            while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (C.rec[m].start < M.tend) lo = m + 1; else hi = m; }
            ok = lo > 0 && C.rec[lo - 1].pmaxend > M.tstart;
        }
        if (ok) lv = 1;
    }
    if (gl == 0) live[r] = lv;
}

// ---------------------------------------------------------------------------------------
// k_callable: one wave per read; a word of the bit array = 32 query bases.
// A match base counts when its quality is at least min_bq, it is not trimmed, and the
// number of mismatch-list entries in its window is at most max_mismatch_count; the window
// is the one get_mismatch_range gives for the START of the base's cs match operation,
// shifted along (normcounts.py:84-90), in 0-based coordinates against the 1-based list.
// A substitution always counts (its three tests are evaluated and ignored, :97-109).
//
// Away from every mismatch entry the window test cannot fail and a base's bit is its quality test and its trim test, so
// the kernel runs in two passes.  Pass A streams the read's qualities once (their sum decides the read filter's mean
// quality, normcounts.py:302, bamlib.py:34-36: it is the kernel that reads every quality anyway), 32 bases a lane, and
// writes quality-and-trim words for the whole read.  Pass B takes the words that lie within two windows of a mismatch entry --
// marked beforehand in a bitmap, from the segment boundaries (indels) and the substitutions, a twentieth of the words -- 64
// at a time, a lane each, with the exact rule.  A read that fails a filter gets zeros: it is piled, not counted; a read that
// stays is counted (num_ccs: ccs_flag, unless the run is phased -- k_pair_ccs then).
constexpr int CAL_NM = 256;     // mismatch entries kept in LDS per wave
constexpr int CAL_BM = 64;      // dwords of the bitmap of words to redo: reads of up to 65,536 bases (a longer one: every word exact)
constexpr int CAL_LIST = 128;   // words gathered before a round of pass B

// A read's segment and mismatch lists, in LDS when they fit there (nearly always) or in memory: two types with
// address-space-qualified pointers, chosen once per wave.  (A choice per access -- `k < CAL_NM ? lds[k] : mem[k]` through
// generic pointers -- is compiled into a select between the two POINTERS and a flat load; the chain of those in the
// binary searches made pass B more than half of this kernel's time.)
typedef int cal_v4i __attribute__((ext_vector_type(4)));
struct CalListsLds {
    const __attribute__((address_space(3))) int32_t* mis;
    const __attribute__((address_space(3))) uint32_t* mq;
    const __attribute__((address_space(3))) cal_v4i* seg;
    __device__ __forceinline__ int32_t MIS(int k) const { return mis[k]; }
    __device__ __forceinline__ uint32_t MQ(int k) const { return mq[k]; }
    __device__ __forceinline__ int4 SEG(int j) const { const cal_v4i v = seg[j]; return make_int4(v.x, v.y, v.z, v.w); }
};
struct CalListsMem {
    const __attribute__((address_space(1))) int32_t* mis;
    const __attribute__((address_space(1))) uint32_t* mq;
    const __attribute__((address_space(1))) cal_v4i* seg;
    __device__ __forceinline__ int32_t MIS(int k) const { return mis[k]; }
    __device__ __forceinline__ uint32_t MQ(int k) const { return mq[k]; }
    __device__ __forceinline__ int4 SEG(int j) const { const cal_v4i v = seg[j]; return make_int4(v.x, v.y, v.z, v.w); }
};

// What the tests of one read need (wave-uniform).
struct CalRead {
    const __attribute__((address_space(1))) uint8_t* bq;      // the read's qualities
    __attribute__((address_space(1))) uint32_t* words;        // the read's words of the bit array
    const __attribute__((address_space(1))) uint32_t* nq_top; // N-reference substitutions: query offsets at nq_top[-k] >> 5, ascending
    int32_t qlen, qstart, ns, nm, nN;
    int32_t w, maxmm, min_bq, min_bq_c, trim_lo, trim_hi;

    __device__ __forceinline__ int32_t NQ(int k) const { return (int32_t)(nq_top[-k] >> 5); }

    // the quality and trim tests of the 32 bases from qa on, given their qualities (bytes behind the read are masked by the trim)
    __device__ __forceinline__ uint32_t quality_trim(const uint32_t (&bw)[8], int32_t qa) const {
        uint32_t okq = 0;    // four bytes at a time: the low seven bits compared, bit 7 by itself
        const uint32_t hb = (bw[0] | bw[1] | bw[2] | bw[3] | bw[4] | bw[5] | bw[6] | bw[7]) & 0x80808080u;   // a quality of 128 or more among them
        if (min_bq <= 127 && !hb) {
#pragma unroll
            for (int k = 0; k < 8; k++) okq |= cs_pack4(cs_ge_bytes(bw[k], (uint32_t)min_bq_c)) << (4 * k);
        } else if (min_bq <= 127) {
#pragma unroll
            for (int k = 0; k < 8; k++)
                okq |= cs_pack4(cs_ge_bytes(bw[k] & 0x7f7f7f7fu, (uint32_t)min_bq_c) | (bw[k] & 0x80808080u)) << (4 * k);
        } else if (min_bq <= 255) {                           // (a threshold above 127: only a quality of 128 or more can pass)
#pragma unroll
            for (int k = 0; k < 8; k++)
                okq |= cs_pack4((min_bq > 128 ? cs_ge_bytes(bw[k] & 0x7f7f7f7fu, (uint32_t)(min_bq - 128)) : 0x80808080u) &
                                (bw[k] & 0x80808080u)) << (4 * k);
        }
        if (min_bq <= 0) okq = ~0u;
        // not trimmed and not soft-clipped: trim_lo <= q <= trim_hi (the two bounds are whole numbers), and q < qlen
        const int32_t lo_q = max(trim_lo, 0), hi_q = min(trim_hi, qlen - 1);
        const int32_t a0 = max(lo_q - qa, 0), a1 = min(hi_q - qa, 31);
        return okq & ((a0 <= a1) ? ((a1 - a0 >= 31 ? ~0u : ((1u << (a1 - a0 + 1)) - 1u)) << a0) : 0u);
    }

    // Which words lie within two windows of a mismatch entry: around every segment boundary (an indel: from the last base in
    // front of it to the first base behind it) and every substitution, in query coordinates.  (A base and an entry that are
    // D reference positions apart with no indel between them are D query bases apart; with indels between them the nearest
    // of those is an entry itself and no further from the base.)  2 w + 2 either way: a base's window reaches w reference
    // positions to each side, up to 2 w to one side where its match operation starts near an end of the read, one more for
    // the 0-based positions against the 1-based list.
    template <class L>
    __device__ __forceinline__ void mark_words(const L& ls, uint32_t* bm, int lane) const {
        const int32_t reach = 2 * w + 2;
        auto mark = [&](int32_t qlo, int32_t qhi) {
            qlo = max(qlo, 0); qhi = min(qhi, qlen - 1);
            for (int32_t wd = qlo >> 5; wd <= (qhi >> 5); wd++) atomicOr(&bm[wd >> 5], 1u << (wd & 31));
        };
        for (int j = lane - 1; j + 1 < ns; j += 64) {             // boundary between segment j and j + 1 (j = -1: in front of the first)
            const int4 sb = ls.SEG(j + 1);
            if (j < 0) { if ((uint32_t)sb.w & SEG_INS) mark(qstart - reach, sb.y + reach); continue; }
            const int4 sa = ls.SEG(j);
            const int32_t qa_end = sa.y + ((((uint32_t)sa.w & SEG_DEL) || sa.z <= 0) ? 0 : sa.z);
            mark(qa_end - 1 - reach, sb.y + reach);
        }
        for (int k = lane; k < nm; k += 64) { const uint32_t v = ls.MQ(k); if (v & 16u) { const int32_t q = (int32_t)(v >> 5); mark(q - reach, q + reach); } }
        for (int k = lane; k < nN; k += 64) { const int32_t q = NQ(k); mark(q - reach, q + reach); }
    }

    // Pass B: the word whose first base is qa, the exact way.
    template <class L>
    __device__ __forceinline__ void exact_word(const L& ls, int32_t qa) const {
        auto lower = [&](int32_t x) { int lo = 0, hi = nm; while (lo < hi) { const int m = (lo + hi) >> 1; if (ls.MIS(m) < x) lo = m + 1; else hi = m; } return lo; };
        auto upper = [&](int32_t x) { int lo = 0, hi = nm; while (lo < hi) { const int m = (lo + hi) >> 1; if (x < ls.MIS(m)) hi = m; else lo = m + 1; } return lo; };
        uint32_t bw[8];
        {
            typedef unsigned int v4u __attribute__((ext_vector_type(4)));
            const v4u b0 = *reinterpret_cast<const __attribute__((address_space(1))) v4u*>(bq + qa);
            const v4u b1 = *reinterpret_cast<const __attribute__((address_space(1))) v4u*>(bq + qa + 16);
            bw[0] = b0.x; bw[1] = b0.y; bw[2] = b0.z; bw[3] = b0.w; bw[4] = b1.x; bw[5] = b1.y; bw[6] = b1.z; bw[7] = b1.w;
        }
        const uint32_t okq = quality_trim(bw, qa);
        uint32_t word = 0;
        // the first segment that reaches behind qa (segments are in query order)
        int jc = 0;
        {
            int lo = 0, hi = ns;
            while (lo < hi) {
                const int m = (lo + hi) >> 1;
                const int4 sg = ls.SEG(m);
                const int32_t qspan = (((uint32_t)sg.w & SEG_DEL) || sg.z <= 0) ? 0 : sg.z;
                if (sg.y + qspan <= qa) lo = m + 1; else hi = m;
            }
            jc = lo;
        }
        for (int j = jc; j < ns; j++) {
            const int4 sg = ls.SEG(j);
            if (sg.y >= qa + 32) break;
            if (((uint32_t)sg.w & SEG_DEL) || sg.z <= 0) continue;
            const int32_t a = max(sg.y, qa), b = min(sg.y + sg.z, qa + 32);     // query overlap
            if (a >= b) continue;
            const int32_t tlo = sg.x + (a - sg.y), thi = sg.x + (b - 1 - sg.y);  // 0-based reference positions
            uint32_t nsub_bits = 0;      // N-reference substitutions among these bases; the last one in front of them
            int32_t nsub_prev = -1;
            for (int k = 0; k < nN; k++) {
                const int32_t q = NQ(k);
                if (q >= a && q < b) nsub_bits |= 1u << (q - qa);
                else if (q >= sg.y && q < a) nsub_prev = q;
            }
            // any list entry that could fall into a window of these bases?
            const int k0 = lower(tlo - 2 * w - 1);
            if (k0 >= nm || ls.MIS(k0) > thi + 2 * w + 1) {
                word |= (okq & (((b - a) >= 32 ? ~0u : ((1u << (b - a)) - 1u)) << (a - qa))) | nsub_bits;
                continue;
            }
            // the few entries near these bases, in registers (value, query offset | substitution flag); a lane with more
            // than NE nearby takes the exact loop over its bases below
            constexpr int NE = 4;
            int32_t ev[NE];
            uint32_t eq[NE];
            int ne = 0;
#pragma unroll
            for (int i = 0; i < NE; i++) {
                ev[i] = 0x7fffffff; eq[i] = 0;
                if (k0 + i < nm) { const int32_t m = ls.MIS(k0 + i); if (m <= thi + 2 * w + 1) { ev[i] = m; eq[i] = ls.MQ(k0 + i); ne = i + 1; } }
            }
            const bool overflow = k0 + NE < nm && ls.MIS(k0 + NE) <= thi + 2 * w + 1;   // more than NE entries nearby
            // start of the match operation the first base belongs to: behind the previous substitution of this
            // segment, else the segment start
            int32_t osq = sg.y;
            {
                // the last entry at or in front of the first base: counted among the entries in registers (those in front of
                // them lie further back still), a search only when all NE of them do and there are more
                int le = 0;
#pragma unroll
                for (int i = 0; i < NE; i++) le += (ev[i] <= tlo) ? 1 : 0;
                const int kp = (le == NE && overflow) ? lower(tlo + 1) - 1 : k0 + le - 1;
                if (kp >= 0) {
                    uint32_t pv;
                    if (kp < k0 || kp >= k0 + NE) pv = ls.MQ(kp);
                    else { pv = eq[0];
#pragma unroll
                        for (int i = 1; i < NE; i++) if (kp - k0 == i) pv = eq[i]; }
                    const int32_t pq = (int32_t)(pv >> 5);
                    if ((pv & 16u) && pq >= sg.y && pq < a) osq = pq + 1;
                }
                if (nsub_prev >= 0) osq = max(osq, nsub_prev + 1);
            }
            // "How many entries see this base" as a sum of bit ranges: bit-sliced counters instead of a loop over the
            // bases.  A match operation that starts at least w bases from either end of the read has the window (w, w)
            // (bamlib.py:245-258) -- every operation that starts among these 32 bases, given where the word lies; the one
            // that started in front of them (osq) may begin within w of the read's start and has (osq, 2 w - osq) then: it
            // holds the bases up to the first substitution among them.
            // (Where none of the bases passes its quality and trim tests -- the trimmed ends of the read -- the counts decide
            // nothing and the same code gives the substitutions' bits.)
            const uint32_t span = ((b - a) >= 32 ? ~0u : ((1u << (b - a)) - 1u)) << (a - qa);
            if (!overflow && ((qa >= w && (int64_t)qa + 32 + w <= (int64_t)qlen) || !(okq & span))) {
                const int32_t shift = sg.y - sg.x - qa;           // bit of reference position t = t + shift
                const int32_t ur0 = min(osq, w), dr0 = 2 * w - ur0;
                uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, sub = 0;
#pragma unroll
                for (int i = 0; i < NE; i++) {
                    const int32_t sq = (int32_t)(eq[i] >> 5);
                    if (i < ne && (eq[i] & 16u) && sq >= a && sq < b && ev[i] == sg.x + (sq - sg.y) + 1) sub |= 1u << (sq - qa);
                }
                const uint32_t starts = sub | nsub_bits;          // behind each of these a new operation begins
                const uint32_t old_op = (ur0 == w) ? 0u : starts ? ((1u << __builtin_ctz(starts)) - 1u) : ~0u;
                auto bits_of = [](int lo, int hi) -> uint32_t {
                    lo = max(lo, 0); hi = min(hi, 31);
                    return lo <= hi ? ((hi - lo) >= 31 ? ~0u : ((1u << (hi - lo + 1)) - 1u)) << lo : 0u;
                };
#pragma unroll
                for (int i = 0; i < NE; i++) {
                    if (i >= ne) continue;
                    uint32_t rr = bits_of(ev[i] - w + shift, ev[i] + w + shift);         // base t sees entry e: e - dr <= t <= e + ur
                    if (old_op) rr = (rr & ~old_op) | (bits_of(ev[i] - dr0 + shift, ev[i] + ur0 + shift) & old_op);
                    const uint32_t k0_ = c0 & rr; c0 ^= rr;
                    const uint32_t k1_ = c1 & k0_; c1 ^= k0_;
                    const uint32_t k2_ = c2 & k1_; c2 ^= k1_;
                    c3 ^= k2_;
                }
                uint32_t gt = 0;                                   // bases seen by more than maxmm entries
                if (maxmm < 8) {
                    uint32_t same = ~0u;
                    const uint32_t planes[4] = {c0, c1, c2, c3};
#pragma unroll
                    for (int pbit = 3; pbit >= 0; pbit--) {
                        const uint32_t kb = ((maxmm >> pbit) & 1) ? ~0u : 0u;
                        gt |= same & planes[pbit] & ~kb;
                        same &= ~(planes[pbit] ^ kb);
                    }
                }
                word |= (span & ((okq & ~gt) | sub)) | nsub_bits;
                continue;
            }
            for (int32_t q = a; q < b; q++) {
                const int32_t t = sg.x + (q - sg.y);
                const int bit = q - qa;
                bool is_sub = false;
#pragma unroll
                for (int i = 0; i < NE; i++) if (ev[i] == t + 1 && (eq[i] & 16u) && (int32_t)(eq[i] >> 5) == q) is_sub = true;
                if (overflow && !is_sub)
                    for (int kk = lower(t + 1); kk < nm && ls.MIS(kk) == t + 1; kk++) { const uint32_t v = ls.MQ(kk); if ((v & 16u) && (int32_t)(v >> 5) == q) is_sub = true; }
                if (is_sub || ((nsub_bits >> bit) & 1u)) { word |= 1u << bit; osq = q + 1; continue; }
                int64_t qs = (int64_t)osq - w, qe = (int64_t)osq + w, ur, dr;      // bamlib.py:245-258
                if (qs < 0) { ur = w + qs; dr = w - qs; }
                else if (qe > qlen) { ur = w + (qe - qlen); dr = qlen - osq; }
                else { ur = w; dr = w; }
                int cnt = 0;
                if (!overflow) {
#pragma unroll
                    for (int i = 0; i < NE; i++) cnt += (ev[i] >= t - ur && ev[i] <= t + dr) ? 1 : 0;
                } else cnt = upper((int32_t)(t + dr)) - lower((int32_t)(t - ur));
                if (cnt <= maxmm && ((okq >> bit) & 1u)) word |= 1u << bit;
            }
        }
        words[qa >> 5] = word;
    }
};

__global__ void __launch_bounds__(256) k_callable(Reads R, Derived D, Params P, uint8_t* live, uint32_t* cbits, uint8_t* ccs_flag) {
    __shared__ int32_t s_mis[4][CAL_NM];
    __shared__ uint32_t s_mq[4][CAL_NM];
    __shared__ __align__(16) int4 s_seg[4][64];
    __shared__ uint32_t s_bm[4][CAL_BM];
    __shared__ uint16_t s_list[4][CAL_LIST];
    const int lane = threadIdx.x & 63, wv = uni((int)(threadIdx.x >> 6));
    const int64_t r = (int64_t)blockIdx.x * 4 + wv;
    if (r >= R.n) return;
    const int64_t qo = uni(R.qoff[r]);
    const int32_t qlen = uni(R.qlen[r]);
    if (!uni((int)live[r])) {                                  // no base of it counts (every read's words are written: the array is not cleared first)
        for (int32_t o = lane * 32; o < qlen; o += 2048) cbits[(qo + o) >> 5] = 0;
        return;
    }
    const ReadMeta Mv = D.meta[r];
    const int ns = uni(Mv.nseg);
    const int64_t segbase = uni(Mv.segbase);
    const int nm = uni(D.nmis[r]);
    const Seg* gsegs = D.segs + segbase;
    const int32_t* gmis = D.mis + segbase;
    const uint32_t* gmq = D.mq + segbase;
    uint32_t* bm = s_bm[wv];
    uint16_t* list = s_list[wv];
    const bool in_lds = nm <= CAL_NM && ns <= 64;              // (the wave's choice, made once)
    if (in_lds) {
        for (int k = lane; k < nm; k += 64) { s_mis[wv][k] = gmis[k]; s_mq[wv][k] = gmq[k]; }
        if (lane < ns) s_seg[wv][lane] = *reinterpret_cast<const int4*>(gsegs + lane);
    }
    bm[lane] = 0;
    __builtin_amdgcn_wave_barrier();
    CalListsLds ll;
    ll.mis = (const __attribute__((address_space(3))) int32_t*)s_mis[wv];
    ll.mq = (const __attribute__((address_space(3))) uint32_t*)s_mq[wv];
    ll.seg = (const __attribute__((address_space(3))) cal_v4i*)s_seg[wv];
    CalListsMem lm;
    lm.mis = (const __attribute__((address_space(1))) int32_t*)gmis;
    lm.mq = (const __attribute__((address_space(1))) uint32_t*)gmq;
    lm.seg = (const __attribute__((address_space(1))) cal_v4i*)gsegs;
    CalRead cr;
    cr.bq = (const __attribute__((address_space(1))) uint8_t*)(R.bq + qo);
    cr.words = (__attribute__((address_space(1))) uint32_t*)(cbits + (qo >> 5));
    // substitutions with an N reference base (rare): not in the mismatch list, their bases always count, and each one
    // starts a new match operation behind it (normcounts.py:75-110 walks the cs operations).  Query offsets, ascending.
    cr.nN = uni(D.nnsub[r]);
    cr.nq_top = (const __attribute__((address_space(1))) uint32_t*)(gmq + ((uni(R.cs_off[r + 1]) >> 1) - (uni(R.cs_off[r]) >> 1)));
    cr.qlen = qlen; cr.qstart = uni(R.qstart[r]); cr.ns = ns; cr.nm = nm;
    cr.w = P.p.mismatch_window_size; cr.maxmm = P.p.max_mismatch_count;
    cr.min_bq = P.p.min_bq; cr.min_bq_c = min(max(cr.min_bq, 1), 127);
    // (the two trim bounds, cut to the aligned part of the query: a soft-clipped base is no base of any cs operation and
    //  never counts, and no mismatch entry is near enough to send its word through pass B)
    int32_t q_al_end = cr.qstart;
    if (ns > 0) { const Seg sl = gsegs[ns - 1]; q_al_end = sl.q0 + (((sl.flags & SEG_DEL) || sl.len <= 0) ? 0 : sl.len); }
    cr.trim_lo = max((int32_t)floor(P.p.min_trim * (double)qlen), cr.qstart);
    cr.trim_hi = min((int32_t)ceil((1.0 - P.p.min_trim) * (double)qlen), uni(q_al_end) - 1);
    const int32_t nwords = (qlen + 31) >> 5;
    const bool big = nwords > CAL_BM * 32;                      // a read the bitmap does not hold: every word the exact way

    if (!big) { if (in_lds) cr.mark_words(ll, bm, lane); else cr.mark_words(lm, bm, lane); }
    __builtin_amdgcn_wave_barrier();

    // ---- pass A: the qualities once; quality-and-trim words everywhere
    uint32_t qsum = 0;   // this lane's share of the sum of the read's qualities (from offset 0: the mean is over the whole query)
    {
        const int32_t q_last = (max(qlen, 1) - 1) & ~31;       // (addresses clamped into the read)
        uint4 p0, p1;
        {
            const int32_t qn = min(lane * 32, q_last);
            p0 = *reinterpret_cast<const uint4*>(R.bq + qo + qn);
            p1 = *reinterpret_cast<const uint4*>(R.bq + qo + qn + 16);
        }
        for (int32_t c0 = 0; c0 < qlen; c0 += 2048) {
            const int32_t qa = c0 + lane * 32;
            const uint4 b0 = p0, b1 = p1;
            {                                                   // the next window's qualities are asked for before this one is worked on
                const int32_t qn = min(c0 + 2048 + lane * 32, q_last);
                p0 = *reinterpret_cast<const uint4*>(R.bq + qo + qn);
                p1 = *reinterpret_cast<const uint4*>(R.bq + qo + qn + 16);
            }
            if (qa < qlen) {
                const uint32_t bw[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
                if (qa + 32 <= qlen) {
#pragma unroll
                    for (int k = 0; k < 8; k++) qsum = __builtin_amdgcn_sad_u8(bw[k], 0u, qsum);
                } else {                                          // the read's last bases: the bytes behind them are padding
#pragma unroll
                    for (int k = 0; k < 8; k++) {
                        const int rb = qlen - (qa + 4 * k);       // bytes of the word inside the read
                        const uint32_t x = rb >= 4 ? bw[k] : rb <= 0 ? 0u : (bw[k] & (0xffffffffu >> (8 * (4 - rb))));
                        qsum = __builtin_amdgcn_sad_u8(x, 0u, qsum);
                    }
                }
                cbits[(qo + qa) >> 5] = cr.quality_trim(bw, qa);
            }
        }
    }

    // ---- pass B: the words with a mismatch entry nearby (every word of a read the bitmap does not hold), gathered into a
    //      list and worked off 64 at a time, a lane each.  One place in the code for each of the two kinds of lists.
    const int ndw = (nwords + 31) >> 5;
    for (int32_t next = 0;;) {                                  // next: the bitmap dword (big: the word) to go on from
        int nl = 0;
        if (big) {
            nl = min(CAL_LIST, nwords - next);
            for (int i = lane; i < nl; i += 64) list[i] = (uint16_t)i;      // (offsets from `next`: a word number may not fit 16 bits)
        } else {
            for (; next < ndw; next += 2) {
                const uint64_t bits2 = (uint64_t)uni(bm[next]) | ((uint64_t)(next + 1 < ndw ? uni(bm[next + 1]) : 0u) << 32);
                if (!bits2) continue;
                const int here = __builtin_popcountll(bits2);
                if (nl + here > CAL_LIST) break;
                if ((bits2 >> lane) & 1ull) {
                    const int rank = __builtin_popcountll(bits2 & ((1ull << lane) - 1ull));
                    const int32_t wd = next * 32 + lane;
                    list[nl + rank] = (uint16_t)min(wd, nwords - 1);
                }
                nl += here;
            }
        }
        if (nl <= 0) break;
        __builtin_amdgcn_wave_barrier();
        const int32_t wbase = big ? next : 0;
        if (in_lds) { for (int i0 = 0; i0 < nl; i0 += 64) if (i0 + lane < nl) cr.exact_word(ll, (wbase + (int32_t)list[i0 + lane]) * 32); }
        else { for (int i0 = 0; i0 < nl; i0 += 64) if (i0 + lane < nl) cr.exact_word(lm, (wbase + (int32_t)list[i0 + lane]) * 32); }
        __builtin_amdgcn_wave_barrier();
        if (big) next += nl;
    }
    // ---- the mean quality (np.mean of the whole query against min_qv, as in k_read_live's other tests)
    const uint32_t qtot = (uint32_t)lane_val(wave_incl_add((int)qsum, lane), 63);
    if ((double)qtot / (double)qlen < (double)P.p.min_qv) {
        if (lane == 0) live[r] = 0;
        for (int32_t o = lane * 32; o < qlen; o += 2048) cbits[(qo + o) >> 5] = 0;     // no base of it counts
    } else if (!P.p.phase && lane == 0) ccs_flag[R.qid[r]] = 1;
}

// ---------------------------------------------------------------------------------------
// k_norm_tile: the tile sweep of himut_sweep.h, counters only.  With a list (launched behind k_norm_quad): the tiles
// that kernel left alone, any workgroup any tile; a list that did not hold them all is the host's business (it repeats
// the contig without the list).  Without one: every tile of every chunk, a row of the grid per chunk, the tiles dealt
// to the XCD classes.
#ifndef HIMUT_NT_WAVES
#define HIMUT_NT_WAVES 5
#endif

struct NormRedo { int32_t chunk, base; };          // 256 positions from `base` of chunk `chunk`, left to k_norm_tile by k_norm_quad

__global__ void __launch_bounds__(256, HIMUT_NT_WAVES) k_norm_tile(NormArgs A, Derived D, const uint32_t* callable, const int32_t* winlo,
                                                   const int32_t* winhi, int64_t nblk, int64_t tiles_per_class, const NormRedo* redo,
                                                   const unsigned int* nredo, unsigned int redo_cap) {
    __shared__ NormLds L;
    const int64_t nlist = redo ? (int64_t)min(*nredo, redo_cap) : 0;
    if (redo && nlist == 0) return;
    norm_lds_init(L, A);
    const bool phase = A.P.p.phase != 0;
    int bad = 0;
    const int64_t per = redo ? tiles_per_class : norm_tiles_per_class(A, (int)blockIdx.y, tiles_per_class);
    const int64_t wg = redo ? (int64_t)blockIdx.x + (int64_t)blockIdx.y * gridDim.x : (int64_t)(blockIdx.x >> 3);
    const int64_t wgs = redo ? (int64_t)gridDim.x * gridDim.y : (int64_t)(gridDim.x >> 3);
    for (int64_t t = wg; t < (redo ? nlist : per); t += wgs) {
        const int chunk = redo ? redo[t].chunk : (int)blockIdx.y;
        const int32_t cs_ = A.C.start[chunk], ce_ = A.C.end[chunk];
        const int64_t tile = (int64_t)(blockIdx.x & 7) * per + t;
        const int64_t base = redo ? (int64_t)redo[t].base : (int64_t)cs_ + tile * 256;
        if (base >= ce_) { if (redo) continue; break; }           // the same for every thread
        const NormTile T = norm_tile_at(A, chunk, base, cs_, ce_, winlo, winhi, nblk, phase, bad);
        NormPos p;
        norm_sweep_tile(L, A, D, callable, T, p, phase, bad);
        if (!T.valid) continue;
        norm_tally(norm_classify(p, A, L.tally, T.ref, T.rpos, phase, bad), p.tri_sum, A, L.tally, T.rpos, T.refc);
    }
    norm_flush(L.tally, A, bad);
}

// ---------------------------------------------------------------------------------------
// A position k_norm_quad does not classify itself -- its column holds a base of another allele than the reference's, or
// hom-ref is not the smallest of its genotype sums by itself: everything the column walk knows about it.  One position in
// thirty; k_norm_dirty takes them a lane each, where inside k_norm_quad the general classification would run for a lane or
// two of a wave, every other wave, and set the kernel's registers.
struct NormDirty {
    int64_t rpos;
    uint32_t nref, tri_sum, n_ins, n_del, h0, h1;
    uint32_t cnt[4];          // bases of A, T, G, C that are not the reference allele's
    double R[3];              // the reference allele's three sums
    double S[9];              // [table * 3 + slot]: the other alleles', allele c in slot c - (c > ref)
};

__global__ void __launch_bounds__(256) k_norm_dirty(NormArgs A, const NormDirty* recs, const uint32_t* dcount, const int64_t* doff, int64_t nregions) {
    __shared__ NormTally tally;
    norm_tally_init(tally, A);
    __syncthreads();
    const int tid = threadIdx.x;
    const bool phase = A.P.p.phase != 0;
    int bad = 0;
    // the list is in `nregions` parts, part r in entries [doff[r], doff[r + 1]) (one part per workgroup of the sweep, filled
    // from its start, a third full or less): a wave per part
    const int lane = tid & 63;
    for (int64_t region = ((int64_t)blockIdx.x * 256 + tid) >> 6; region < nregions; region += (int64_t)gridDim.x * 4)
    for (int64_t i = lane; i < (int64_t)min((int64_t)dcount[region], doff[region + 1] - doff[region]); i += 64) {
        const int64_t t = doff[region] + i;
        const NormDirty d = recs[t];
        const int refc = (int)A.refseq[d.rpos];
        const int ref = char2allele(refc);
        NormPos p;
        p.cnt[0] = d.cnt[0]; p.cnt[1] = d.cnt[1]; p.cnt[2] = d.cnt[2]; p.cnt[3] = d.cnt[3]; p.cnt[4] = d.n_ins; p.cnt[5] = d.n_del;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int a = max(min(b - (b > ref ? 1 : 0), 2), 0);     // (the reference allele's own entries are replaced in the classification)
            double v0 = d.S[0], v1 = d.S[3], v2 = d.S[6];
            if (a == 1) { v0 = d.S[1]; v1 = d.S[4]; v2 = d.S[7]; }
            if (a == 2) { v0 = d.S[2]; v1 = d.S[5]; v2 = d.S[8]; }
            p.S[0][b] = v0; p.S[1][b] = v1; p.S[2][b] = v2;
        }
        p.R0 = d.R[0]; p.R1 = d.R[1]; p.R2 = d.R[2];
        p.nref = d.nref; p.tri_sum = d.tri_sum; p.h0 = d.h0; p.h1 = d.h1;
        p.bq0 = false;                                                // (a zero quality ended the column in k_norm_quad)
        norm_tally(norm_classify(p, A, tally, ref, d.rpos, phase, bad), p.tri_sum, A, tally, d.rpos, refc);
    }
    norm_flush(tally, A, bad);
}

}  // namespace himut
