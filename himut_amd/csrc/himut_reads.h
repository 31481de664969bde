// Read-pass kernels of libhimut_hip.so that more than one pipeline launches (himut_call.hip launches them all):
//
//   k_flag_bases       which reads hold a base outside ATGC (once per pushed batch)
//   k_parse_cs         one wave per read, a wave-parallel tokenizer: cs tag -> gapless segments + mismatch list +
//                      identity (cslib.py:7-64, bamlib.py:47-63); on the call path it also sets the bitmap of column
//                      positions and stores its share of the EMPTY column store
//   k_check_longcs     long-form cs tags against SEQ
//   k_read_hap         (--phase) sixteen lanes per (chunk, read), a lane per hetSNP: haplib.py:46-83
//   k_window_index     per 256-position block: the range of reads that can cover it
//   k_count_flags      the number of flagged reads
#pragma once

#include "himut_device.h"

namespace himut {

// ---------------------------------------------------------------------------------------
// k_flag_bases: which reads hold a base outside ATGC anywhere in SEQ -- the reference's pile raises KeyError on one that is
// aligned (caller.py:57, util.py:17), wherever it sits in a fetched read.  The packed bases are read once per pushed batch
// (like the window index, the answer depends on the reads only); a flagged read -- CCS reads do not carry N -- is then
// looked at base by base, per run, by the kernel that knows what is aligned and what is fetched (aligned_bases_ok).
// One wave per read, 32 bases a lane and step; a BAM code is one of A C G T exactly when it has one bit set.
__global__ void __launch_bounds__(256) k_flag_bases(int64_t n, const int64_t* qoff, const int32_t* qlen, const uint8_t* seq, uint8_t* out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int64_t qo = __builtin_amdgcn_readfirstlane((int)(qoff[r] >> 32)) * 4294967296ll + (uint32_t)__builtin_amdgcn_readfirstlane((int)qoff[r]);
    const int32_t ql = __builtin_amdgcn_readfirstlane(qlen[r]);
    uint32_t badw = 0;
    for (int32_t o = lane * 32; o < ql; o += 2048) {
        const uint4 v = *reinterpret_cast<const uint4*>(seq + ((qo + o) >> 1));      // (a read's bases start at a multiple of 32)
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t x = w[k];
            const int left = ql - (o + 8 * k);                   // bases of the word inside the read (byte i: bases 2i, 2i + 1, high nibble first)
            if (left <= 0) continue;
            uint32_t pc = x - ((x >> 1) & 0x55555555u);
            pc = (pc & 0x33333333u) + ((pc >> 2) & 0x33333333u);   // bits set, per nibble
            uint32_t d = pc ^ 0x11111111u;
            if (left < 8) {                                      // nibbles behind the read's last base do not count
                uint32_t keep = 0;
                for (int b = 0; b < left; b++) keep |= 0xfu << (8 * (b >> 1) + ((b & 1) ? 0 : 4));
                d &= keep;
            }
            badw |= d;
        }
    }
    const unsigned long long any = __ballot(badw != 0);
    if (lane == 0) out[r] = any ? 1 : 0;
}

// ---------------------------------------------------------------------------------------
// bq_issue / bq_finish: the wave streams its read's qualities with 16-byte coalesced loads, eight in flight
// (np.mean of the whole query, bamlib.py:34-36).  k_parse_cs issues the first eight rows before it decodes
// the cs tag and sums after it.
constexpr int BQ_AHEAD = 4;   // rows of 1 KB issued ahead of the decode

struct BqAhead {            // the first rows of a read's qualities, in flight while the wave decodes its cs tag
    uint4 v[BQ_AHEAD];
    const uint8_t* base;   // this lane's 16 bytes of row 0
    int n, npre;           // quality bytes of the read; whole 1 KB rows among the BQ_AHEAD (the others were clamped loads)
};

__device__ __forceinline__ void bq_issue(const Reads& R, int64_t r, int lane, BqAhead& A) {
    const uint8_t* row0 = R.bq + uni(R.qoff[r]);
    A.base = row0 + lane * 16;
    A.n = uni(R.qlen[r]);
    A.npre = min(BQ_AHEAD, A.n >> 10);
#pragma unroll
    for (int k = 0; k < BQ_AHEAD; k++)                   // a row past the whole ones: reload the read's first bytes (always there)
        A.v[k] = *reinterpret_cast<const uint4*>(k < A.npre ? A.base + k * 1024 : row0);
}

__device__ __forceinline__ void bq_finish(const BqAhead& A, int64_t r, int lane, uint32_t* bqsum) {
    const uint8_t* base = A.base;
    const int n = A.n;
    uint32_t sum = 0;
    const int nfull = n & ~1023;                 // whole 1 KB steps: four byte sums per lane and step
#define BQ_ADD(V) do { sum = __builtin_amdgcn_sad_u8(V.x, 0u, sum); sum = __builtin_amdgcn_sad_u8(V.y, 0u, sum); \
        sum = __builtin_amdgcn_sad_u8(V.z, 0u, sum); sum = __builtin_amdgcn_sad_u8(V.w, 0u, sum); } while (0)
#pragma unroll
    for (int k = 0; k < BQ_AHEAD; k++) if (k < A.npre) BQ_ADD(A.v[k]);
    int o = A.npre * 1024;
    for (; o + 8192 <= nfull; o += 8192) {       // eight loads in flight per lane
        const uint4 a = *reinterpret_cast<const uint4*>(base + o);
        const uint4 b = *reinterpret_cast<const uint4*>(base + o + 1024);
        const uint4 c = *reinterpret_cast<const uint4*>(base + o + 2048);
        const uint4 d = *reinterpret_cast<const uint4*>(base + o + 3072);
        const uint4 e = *reinterpret_cast<const uint4*>(base + o + 4096);
        const uint4 f = *reinterpret_cast<const uint4*>(base + o + 5120);
        const uint4 g = *reinterpret_cast<const uint4*>(base + o + 6144);
        const uint4 h = *reinterpret_cast<const uint4*>(base + o + 7168);
        BQ_ADD(a); BQ_ADD(b); BQ_ADD(c); BQ_ADD(d); BQ_ADD(e); BQ_ADD(f); BQ_ADD(g); BQ_ADD(h);
    }
    for (; o + 4096 <= nfull; o += 4096) {       // four loads in flight per lane
        const uint4 a = *reinterpret_cast<const uint4*>(base + o);
        const uint4 b = *reinterpret_cast<const uint4*>(base + o + 1024);
        const uint4 c = *reinterpret_cast<const uint4*>(base + o + 2048);
        const uint4 d = *reinterpret_cast<const uint4*>(base + o + 3072);
        BQ_ADD(a); BQ_ADD(b); BQ_ADD(c); BQ_ADD(d);
    }
    for (; o < nfull; o += 1024) {
        const uint4 a = *reinterpret_cast<const uint4*>(base + o);
        BQ_ADD(a);
    }
#undef BQ_ADD
    if (nfull + lane * 16 < n) {                 // the last, partial step: bytes behind the read are masked off
        const uint4 v = *reinterpret_cast<const uint4*>(base + nfull);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int rem = n - (nfull + lane * 16 + 4 * k);
            uint32_t x = w[k];
            if (rem < 4) x = rem <= 0 ? 0u : (x & (0xffffffffu >> (8 * (4 - rem))));
            sum = __builtin_amdgcn_sad_u8(x, 0u, sum);
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
    if (lane == 0) bqsum[r] = sum;
}

// ---------------------------------------------------------------------------------------
// k_parse_cs: one WAVE per read, a wave-parallel cs tokenizer.
//
// The tag is consumed 1 KB per step, 16 bytes per lane.  Operation starts are the bytes
// ':' '*' '+' '-' '=' (the alternatives of the reference's regex, cslib.py:8; payload bytes
// are digits or letters and can never be one of them), found by every lane in its own 16
// bytes and compacted into an LDS list with one wave scan.  An operation is complete when
// the NEXT start (or the end of the tag) is known, so lane k takes operation k of the
// list: kind = its first byte, payload = the bytes up to the next start.  Reference and
// query offsets are wave prefix sums of the per-operation advances; the mismatch list
// (cslib.py:47-64) and the gapless segments are written at offsets that come from two more
// scans.  Only a handful of scalars (running offsets, the open aligned run, the unfinished
// last operation) carry from one step to the next.

constexpr int PB = 1024;  // cs bytes per step

// WITH_BQ: the wave also issues the first rows of its read's qualities (bq_issue) behind the first KB of the tag,
// decodes the tag while they are in flight, then sums the qualities (bq_finish): waves in that phase are bound by
// HBM, waves in the decode by VALU, and a CU holds both kinds at any time.  No caller asks for it any more: the call
// path takes the sum from k_stream_capture and normcounts from k_callable, which stream the qualities anyway, and
// the edge counts and the dense pile never looked at it (0.24 ms a contig each).
//
// posbits (call path; else null): the bitmap of reference positions at which a column must be captured = every
// substitution of every read that passes the filters known before the qualities have been streamed (identity,
// mapq, qlen: caller.py:312-317).  A superset of the candidate positions -- the whole-read quality mean
// (caller.py:310), the trim and mismatch-window filters and the chunk rules only take proposals away (propose_read,
// the tail of the capture wave, which knows the mean by then) -- and nearly equal to them.  The wave keeps the
// positions of its read in LDS and sets the bits once the identity is known (a read with more substitutions than
// the list holds sets them as it goes: a superset is all that is asked for); the atomics cost the decode nothing,
// it is bound by instruction issue.
constexpr int MARK_CAP = 128;

// The decode is bound by latency (a chain of three memory round trips per wave times the waves a CU holds), and what
// limits the waves is the scalar registers: the values the wave keeps uniform.  256-thread workgroups are admitted
// per CU up to 800 / (ceil(sgpr / 16) * 16 + 16) (MI355X_MICROARCH.md): 80 scalars give 8, the 106 the compiler takes
// unasked give 6 -- the cap costs a few spills to vector lanes and is worth a tenth of the kernel.
#ifndef HIMUT_PARSE_SGPR
#define HIMUT_PARSE_SGPR 80
#endif
template <bool WITH_BQ>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(HIMUT_PARSE_SGPR)))
k_parse_cs(Reads R, Derived D, Params P, int* err, uint8_t* ccs, uint32_t* posbits,
                                                  int64_t nposwords, uint4* fill, int64_t fill16, int fill_per) {
    __shared__ __align__(16) uint8_t s_txt[4][32 + PB + 32];   // 32 bytes of the previous step, then this step
    __shared__ uint16_t s_start[4][PB + 8];                      // operation starts, relative to the step (an operation carried
                                                                 // over from an earlier step keeps its start in a register)
    __shared__ int32_t s_mark[4][MARK_CAP];                      // substitution positions of the read (0-based)
    const int tid = threadIdx.x, lane = tid & 63, wv = uni(tid >> 6);
    const int64_t r = (int64_t)blockIdx.x * 4 + wv;
    if (r >= R.n) return;
    // The column store must be EMPTY before the capture writes into it (fill: its fill16 16-byte pieces, or null).  The
    // decode is bound by latency and leaves the memory system idle: every wave stores its share, fill_per pieces per lane,
    // and neither a fill between the decode and the capture nor a second stream is needed.
    if (fill) {
        const uint4 e = make_uint4(0x00070007u, 0x00070007u, 0x00070007u, 0x00070007u);   // CELL_EMPTY
        const int64_t f0 = r * 64 * fill_per;
        for (int k = 0; k < fill_per; k++) { const int64_t o = f0 + 64 * k + lane; if (o < fill16) fill[o] = e; }
    }
    if (lane == 0) ccs[r] = 0;               // the flag propose_read raises for a read that may propose (num_ccs)
    const int64_t cs0 = uni(R.cs_off[r]);
    const int64_t sb = (cs0 >> 1) + r;
    ReadMeta M;
    M.tstart = uni(R.tstart[r]); M.tend = uni(R.tend[r]); M.nseg = 0; M.flags = 0; M.segbase = sb; M.qoff = uni(R.qoff[r]);
    if (uni((int)R.flag[r]) & 0x100) {  // bamlib.py:17
        if (lane == 0) {
            M.flags = RF_SECONDARY;
            D.rflag[r] = RF_SECONDARY; D.nseg[r] = 0; D.nmis[r] = 0; D.nnsub[r] = 0; D.meta[r] = M;
        }
        return;
    }
    const int n = (int)(uni(R.cs_off[r + 1]) - cs0);
    const uint8_t* cs = R.cs + cs0;
    uint8_t* txt = s_txt[wv];
    uint16_t* starts = s_start[wv];
    Seg* segs = D.segs + sb;
    int32_t* mis = D.mis + sb;
    uint32_t* mq = D.mq + sb;
    const int32_t qlen = uni(R.qlen[r]);
    int32_t* marks = s_mark[wv];
    int nmark = 0;
    int nN = 0;                                                          // substitutions with an N reference base
    const int64_t top = (uni(R.cs_off[r + 1]) >> 1) - (cs0 >> 1);        // the read's last slot (an operation takes >= 2 bytes)
    const bool mark = posbits != nullptr && !(uni((int)R.mapq[r]) < P.p.min_mapq) &&
                      (P.p.qlen_lower_limit < qlen && qlen < P.p.qlen_upper_limit);       // caller.py:312-317
    auto flush_marks = [&]() {
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < nmark; i += 64) {
            const int32_t p = marks[i];
            if (p >= 0 && (int64_t)(p >> 5) < nposwords) atomicOr(posbits + (p >> 5), 1u << (p & 31));
        }
        nmark = 0;
        __builtin_amdgcn_wave_barrier();
    };
    // wave-uniform running state
    int t = M.tstart, q = uni(R.qstart[r]);
    int ns = 0, nm = 0, bad = 0;
    int match = 0, mism = 0;         // per lane; summed over the wave after the last step (a read's reference span fits 31 bits)
    bool have_carry = false; int carry_start = 0, carry_kind = 0;     // unfinished last operation of the previous step
    bool aligned_open = false; int run_t0 = 0, run_q0 = 0; bool run_ins = false;  // the aligned run still growing
    int last_kind = 0;                                                 // kind of the last finished operation
    bool has_long = false;

    // The text is loaded one step ahead, always exactly one load per step at an address that depends on no loaded
    // data (clamped to the last step): with loads inside branches the compiler waits for every load in flight at
    // the join, and the first rows of the qualities are in flight here (bq_issue) while the tag is decoded.
    const int last_base = ((max(n, 1) - 1) / PB) * PB;
    uint4 vcur;
    __builtin_memcpy(&vcur, cs + 16 * lane, 16);                   // himut_push_reads leaves 2 KB of slack behind the text
    BqAhead Q;
    if constexpr (WITH_BQ) bq_issue(R, r, lane, Q);
    for (int base = 0; base < n; base += PB) {
        const int nb = min(PB, n - base);
        // ---- text of this step into LDS, behind the last 32 bytes of the previous step (still in LDS)
        const uint4 v = vcur;
        uint4 pb = make_uint4(0, 0, 0, 0);
        if (lane < 2 && base > 0) pb = *reinterpret_cast<const uint4*>(txt + PB + 16 * lane);
        *reinterpret_cast<uint4*>(txt + 32 + 16 * lane) = v;
        if (lane < 2) *reinterpret_cast<uint4*>(txt + 16 * lane) = pb;
        __builtin_memcpy(&vcur, cs + min(base + PB, last_base) + 16 * lane, 16);
        __builtin_amdgcn_wave_barrier();
        // ---- operation starts in this lane's 16 bytes, four bytes at a time in the registers they came in.  A byte's
        // class comes from two 16-entry tables looked up with v_perm_b32, one by its high nibble (which row of the ASCII
        // table), one by its low nibble (which rows that column belongs to): bit 0 / 1 = an operation's first byte
        // (* + - in row 2, : = in row 3), bits 2..4 = payload (digits, upper case, lower case)
        uint32_t stf[4];                                             // 0x80 in the bytes that start an operation
        {
            const uint32_t words[4] = {v.x, v.y, v.z, v.w};
            const int nhere = min(max(nb - 16 * lane, 0), 16);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t w = words[k];
                const int nv = min(max(nhere - 4 * k, 0), 4);
                const uint32_t inside = nv >= 4 ? 0x80808080u : (0x80808080u & ((1u << (8 * nv)) - 1u));   // bytes of the tag
                const uint32_t rh = __builtin_amdgcn_perm(0x10081008u, 0x06010000u, (w >> 4) & 0x07070707u);
                const uint32_t lo = w & 0x0f0f0f0fu, l7 = lo & 0x07070707u;
                const uint32_t la = __builtin_amdgcn_perm(0x1c1c1c1cu, 0x1c1c1c14u, l7), lb = __builtin_amdgcn_perm(0x08080b08u, 0x091b1c1cu, l7);
                const uint32_t rl = __builtin_amdgcn_perm(lb, la, 0x03020100u | ((lo >> 1) & 0x04040404u));
                const uint32_t r = rh & rl, ascii = ~w & 0x80808080u;
                stf[k] = ((r & 0x03030303u) + 0x7f7f7f7fu) & ascii & inside;
                const uint32_t ok = ((r & 0x1f1f1f1fu) + 0x7f7f7f7fu) & ascii;
                if (~ok & inside) bad = HIMUT_ERR_CS;                // a byte the reference's pattern has no place for
            }
        }
        const int cnt = __popc(stf[0]) + __popc(stf[1]) + __popc(stf[2]) + __popc(stf[3]);
        const int incl = wave_incl_add(cnt, lane);
        const int total = lane_val(incl, 63);
        const int off0 = have_carry ? 1 : 0;
        {
            int w = off0 + incl - cnt;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                uint32_t mk = stf[k];
                while (mk) { const int i = __ffs((int)mk) - 1; mk &= mk - 1; starts[w++] = (uint16_t)(16 * lane + 4 * k + (i >> 3)); }
            }
        }
        const int m = off0 + total;
        const bool last_block = base + PB >= n;
        if (last_block && lane == 0) starts[m] = (uint16_t)(n - base);
        const int nops = last_block ? m : m - 1;
        __builtin_amdgcn_wave_barrier();
        if (base == 0 && (m == 0 || starts[0] != 0)) bad = HIMUT_ERR_CS;   // the tag does not begin with an operation
        if (__ballot(bad != 0)) break;
        // ---- operations, 64 per round
        for (int k0 = 0; k0 < nops; k0 += 64) {
            const int k = k0 + lane;
            const bool valid = k < nops;
            int s = 0, e = 0, kind = 0, len = 0, dt = 0, dq = 0, ref = 0, alt = 0;
            if (valid) {
                s = (k == 0 && have_carry) ? carry_start : base + (int)starts[k];
                e = base + (int)starts[k + 1];
                kind = (k == 0 && have_carry) ? carry_kind : (int)txt[32 + (s - base)];
                len = e - s - 1;
                if (kind == ':') {
                    if (len < 1 || len > 9) bad = HIMUT_ERR_CS;
                    else {
                        int v = 0;
                        for (int i = 0; i < len; i++) {
                            const int c = txt[32 + (s + 1 + i - base)];
                            if (!cs_is_digit(c)) bad = HIMUT_ERR_CS;
                            v = v * 10 + (c - '0');
                        }
                        dt = v; dq = v;
                    }
                } else if (kind == '*') {
                    const int a = txt[32 + (s + 1 - base)], b = (len >= 2) ? (int)txt[32 + (s + 2 - base)] : 0;
                    if (len != 2 || !(a >= 'a' && a <= 'z') || !(b >= 'a' && b <= 'z')) bad = HIMUT_ERR_CS;   // \*[a-z][a-z]
                    ref = a - 32; alt = b - 32;
                    dt = 1; dq = 1;
                } else {
                    if (len < 1) bad = HIMUT_ERR_CS;
                    if (kind == '=') { dt = len; dq = len; }
                    else if (kind == '+') dq = len;
                    else dt = len;
                }
            }
            const bool indel = valid && (kind == '+' || kind == '-');
            const bool sub = valid && kind == '*';
            // reference / query offset of every operation
            const int it = wave_incl_add(dt, lane), iq = wave_incl_add(dq, lane);
            const int tk = t + it - dt, qk = q + iq - dq;           // at the operation
            const int ta = t + it, qa = q + iq;                     // after it
            // previous operation's kind, previous indel in this round
            int prev_kind = __shfl_up(kind, 1, 64);
            if (lane == 0) prev_kind = last_kind;
            const int pidx = wave_incl_max(indel ? lane : -1, lane);
            int Pk = __shfl_up(pidx, 1, 64);
            if (lane == 0) Pk = -1;
            const int src = Pk < 0 ? 0 : Pk;
            const int p_ta = __shfl(ta, src, 64), p_qa = __shfl(qa, src, 64), p_kind = __shfl(kind, src, 64);
            // segments: an indel closes the aligned run before it; a deletion is a segment of its own
            int nseg_here = 0;
            Seg sg_run = {0, 0, 0, 0}, sg_del = {0, 0, 0, 0};
            bool run_before = false;
            if (indel) {
                run_before = Pk >= 0 ? (lane - 1 - Pk) > 0 : (aligned_open || lane > 0);
                if (run_before) {
                    const int rt0 = Pk >= 0 ? p_ta : (aligned_open ? run_t0 : t), rq0 = Pk >= 0 ? p_qa : (aligned_open ? run_q0 : q);
                    const bool rins = Pk >= 0 ? (p_kind == '+') : (aligned_open ? run_ins : (last_kind == '+'));
                    sg_run.t0 = rt0; sg_run.q0 = rq0; sg_run.len = tk - rt0; sg_run.flags = rins ? SEG_INS : 0u;
                    nseg_here++;
                }
                if (kind == '-') {
                    sg_del.t0 = tk; sg_del.q0 = qk; sg_del.len = len; sg_del.flags = SEG_DEL | (prev_kind == '+' ? SEG_INS : 0u);
                    nseg_here++;
                }
                // (an insertion straight behind an insertion -- the tokenizer splits "+a+cg" in two, cslib.py:7-10; an aligner
                //  writes one -- is one more mismatch entry at the same position and no segment of its own: the position
                //  still carries "an insertion precedes", and nothing the reference prints depends on how many)
            }
            const int iseg = wave_rank_incl(nseg_here >= 1) + wave_rank_incl(nseg_here == 2);
            if (nseg_here) {
                int w = ns + iseg - nseg_here;
                if (run_before) segs[w++] = sg_run;
                if (kind == '-') segs[w] = sg_del;
            }
            // mismatch list (cslib.py:54-62): substitutions with a non-N reference base, all indels
            int aa = 0, ra = 0, seq_nib = -1;
            if (sub) {
                aa = char2allele(alt);
                if (aa < 0) bad = HIMUT_ERR_BASE;                    // caller.py:62
                if (ref != 'N') { ra = char2allele(ref); if (ra < 0) bad = HIMUT_ERR_BASE; }   // bamlib.py:188
                // the base cs names must be the base SEQ holds (caller.py:62 takes it from cs, the pile from SEQ).  One
                // random sector of SEQ per substitution: here it is fetched beside a decode that is bound by
                // instruction issue, not by memory
                if (ref != 'N' && !bad) {
                    if (qk < 0 || qk >= qlen) bad = HIMUT_ERR_CS;
                    else seq_nib = nib_at(R.seq, M.qoff + qk);       // looked at when the round is over: the load has the round to arrive
                }
            }
            const bool ismis = indel || (sub && ref != 'N');
            const int imis = wave_rank_incl(ismis);
            if (ismis) {
                const int w = nm + imis - 1;
                mis[w] = tk + 1;
                mq[w] = sub ? (((uint32_t)qk << 5) | 16u | ((uint32_t)(ra & 3) << 2) | (uint32_t)(aa & 3)) : ((uint32_t)qk << 5);
            }
            {   // a substitution whose reference base is N: no mismatch entry, but normcounts counts its base
                const bool nsb = sub && ref == 'N';
                const unsigned long long nb = __ballot(nsb);
                if (nb) {
                    if (nsb) {
                        const int64_t k = nN + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(nb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)nb, 0u));
                        mq[top - k] = ((uint32_t)qk << 5) | 8u;
                    }
                    nN += __popcll(nb);
                }
            }
            if (mark) {
                const bool mk = sub && ref != 'N';
                const unsigned long long mb = __ballot(mk);
                if (mb) {
                    if (nmark + __popcll(mb) > MARK_CAP) flush_marks();
                    if (mk) marks[nmark + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mb, 0u))] = tk;
                    nmark += __popcll(mb);
                }
            }
            // identity counts (bamlib.py:47-63)
            match += (valid && (kind == ':' || kind == '=')) ? dt : 0;
            mism += sub ? 1 : (indel ? len : 0);
            if (__ballot(valid && kind == '=')) has_long = true;
            // ---- carry the round's end state
            const int nvalid = min(64, nops - k0);
            const unsigned long long ib = __ballot(indel);
            t = lane_val(ta, nvalid - 1); q = lane_val(qa, nvalid - 1);
            ns += lane_val(iseg, 63); nm += lane_val(imis, 63);
            if (ib) {
                const int L = 63 - __clzll((long long)ib);
                run_t0 = lane_val(ta, L); run_q0 = lane_val(qa, L); run_ins = lane_val(kind, L) == '+';
                aligned_open = L < nvalid - 1;
            } else if (!aligned_open) {
                // the run opens at the first operation of this round
                run_t0 = lane_val(tk, 0); run_q0 = lane_val(qk, 0); run_ins = last_kind == '+';
                aligned_open = true;
            }
            last_kind = lane_val(kind, nvalid - 1);
            if (seq_nib >= 0) {                                    // the substitutions' bases against SEQ
                const int qa = nib2allele(seq_nib);
                if (qa > 3) bad = HIMUT_ERR_BASE;
                else if (qa != aa) bad = HIMUT_ERR_CS;
            }
            if (__ballot(bad != 0)) break;
        }
        if (__ballot(bad != 0)) break;
        if (!last_block) {
            if (m > 0) {
                have_carry = true;
                carry_start = (m == 1 && off0 == 1) ? carry_start : base + (int)starts[m - 1];
                carry_kind = (m == 1 && off0 == 1) ? carry_kind : (int)txt[32 + (carry_start - base)];
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if constexpr (WITH_BQ) bq_finish(Q, r, lane, D.bqsum);
    // a reduction of the lanes' error codes
    if (__ballot(bad != 0)) bad = lane_val(wave_incl_max(bad, lane), 63);      // (rare; the code with the highest number)
    if (!bad) {
        // end of the tag: close the open run; an insertion at the very end is a marker segment
        if (lane == 0) {
            if (aligned_open) { Seg z = {run_t0, run_q0, t - run_t0, run_ins ? SEG_INS : 0u}; segs[ns] = z; }
            else if (last_kind == '+') { Seg z = {t, q, 0, SEG_INS}; segs[ns] = z; }
        }
        if (aligned_open || last_kind == '+') ns++;
        if (t != M.tend || q > qlen) bad = HIMUT_ERR_CS;   // cs inconsistent with CIGAR / SEQ
    }
    const long long match_all = (long long)lane_val(wave_incl_add(match, lane), 63), mism_all = (long long)lane_val(wave_incl_add(mism, lane), 63);
    // identity filter (bamlib.py:47-63, caller.py:314); the other read filters follow behind the capture
    if (!bad && match_all + mism_all == 0) bad = HIMUT_ERR_CS;     // an empty tag: ZeroDivisionError in the reference (bamlib.py:62)
    const double ident = (double)match_all / (double)(match_all + mism_all);
    const bool ident_ok = !bad && !(ident < P.p.min_sequence_identity);
    if (mark && ident_ok && nmark > 0) flush_marks();
    if (lane == 0) {
        if (bad) { set_err(err, bad); ns = 0; nm = 0; }
        uint8_t fl = 0;
        if (ident_ok) fl = RF_IDENT_OK;
        if (has_long) fl |= RF_LONGCS;
        M.nseg = ns; M.flags = fl;
        D.nseg[r] = ns;
        D.nmis[r] = nm;
        D.nnsub[r] = bad ? 0 : nN;
        D.rflag[r] = fl;
        D.meta[r] = M;
    }
}

// long-form tags ('=' with the matched bases spelled out): the letters must be the bases
// SEQ holds, because the pile takes match bases from SEQ (cslib.py:24 takes them from cs).
// Thread per flagged read; minimap2 --cs=short (what himut asks for) never gets here.
__global__ void __launch_bounds__(256) k_check_longcs(Reads R, Derived D, int* err) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R.n || !(D.rflag[r] & RF_LONGCS)) return;
    const uint8_t* cs = R.cs + R.cs_off[r];
    const int64_t n = R.cs_off[r + 1] - R.cs_off[r];
    int64_t q = R.qstart[r];
    const int64_t qo = R.qoff[r];
    int64_t i = 0;
    while (i < n) {
        const int c = cs[i];
        int64_t j = i + 1;
        while (j < n && !cs_is_start(cs[j])) j++;
        const int64_t len = j - i - 1;
        if (c == ':') { int64_t v = 0; for (int64_t k = i + 1; k < j; k++) v = v * 10 + (cs[k] - '0'); q += v; }
        else if (c == '*') q += 1;
        else if (c == '+') q += len;
        else if (c == '=') {
            for (int64_t k = 0; k < len; k++)
                if (upper(cs[i + 1 + k]) != nib2char(nib_at(R.seq, qo + q + k))) { set_err(err, HIMUT_ERR_CS); return; }
            q += len;
        }
        i = j;
    }
}

// ---------------------------------------------------------------------------------------
// k_read_hap: sixteen lanes per (chunk, read-in-window) pair; haplib.get_ccs_hap (haplib.py:61-83).
__global__ void __launch_bounds__(256) k_read_hap(Reads R, Derived D, Chunks C, Phase H, int* err) {
    // chunk = blockIdx.y; sixteen lanes per (chunk, read) pair, a lane per heterozygous SNP of the chunk's phase set under the
    // read: each finds its segment by a search of its own and fetches its base, instead of one thread walking up to forty
    // of them in turn
    const int64_t c = blockIdx.y;
    const int64_t kin = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;       // the pair's place in the chunk's window
    const int gl = threadIdx.x & 15;
    const int64_t p0 = C.pairoff[c];
    if (kin >= C.pairoff[c + 1] - p0) return;
    const int64_t k = p0 + kin;
    const int64_t r = C.rlo[c] + kin;
    uint8_t hap = HAP_NONE;
    const int32_t s = C.start[c], e = C.end[c];
    const int32_t ts = R.tstart[r], te = R.tend[r];
    if (!(D.rflag[r] & RF_SECONDARY) && ts < e && te > s) {
        const int32_t* hpos = H.hpos;
        const int64_t a = H.off[c], b = H.off[c + 1];
        // bisect_right of the read's start and end among the set's positions (haplib.py:68-69): counted, sixteen at a time
        int n_le_s = 0, n_le_e = 0;
        for (int64_t g = a + gl; g < b; g += 16) { const int32_t hp = hpos[g]; n_le_s += hp <= ts ? 1 : 0; n_le_e += hp <= te ? 1 : 0; }
#pragma unroll
        for (int d = 8; d > 0; d >>= 1) { n_le_s += __shfl_xor(n_le_s, d, 16); n_le_e += __shfl_xor(n_le_e, d, 16); }
        const int64_t idx = a + n_le_s, jdx = a + n_le_e;
        if (jdx - idx >= 2) {
            bool all0 = true, all1 = true, uncovered = false;
            const Seg* segs = D.segs + seg_base(R, r);
            const int ns = D.nseg[r];
            const int64_t qo = R.qoff[r];
            for (int64_t g = idx + gl; g < jdx; g += 16) {
                const int32_t rpos = hpos[g] - 1;
                // the first segment that ends behind rpos (segments are in order and do not overlap)
                int lo = 0, hi = ns;
                while (lo < hi) { const int m = (lo + hi) >> 1; if (rpos >= segs[m].t0 + segs[m].len) lo = m + 1; else hi = m; }
                int qb = 0;  // 0: not in tpos2qbase -> KeyError
                if (lo < ns) {
                    const Seg sg = segs[lo];
                    if (rpos >= sg.t0) {
                        if (sg.flags & SEG_DEL) qb = '-';
                        else qb = nib2char(nib_at(R.seq, qo + sg.q0 + (rpos - sg.t0)));
                    }
                }
                if (qb == 0) { uncovered = true; continue; }
                int bit = '-';
                if (H.href[g] && qb == H.href[g]) bit = '0';        // haplib.py:52-57
                else if (H.halt[g] && qb == H.halt[g]) bit = '1';
                const int h0 = H.hbit[g];
                const int h1 = h0 == '0' ? '1' : (h0 == '1' ? '0' : '-');
                if (bit != h0) all0 = false;
                if (bit != h1) all1 = false;
            }
            // the pair's sixteen lanes agree (they sit in one row of the wave)
            int v0 = all0 ? 1 : 0, v1 = all1 ? 1 : 0, vu = uncovered ? 1 : 0;      // (every lane takes part in every exchange)
#pragma unroll
            for (int d = 8; d > 0; d >>= 1) {
                v0 &= __shfl_xor(v0, d, 16);
                v1 &= __shfl_xor(v1, d, 16);
                vu |= __shfl_xor(vu, d, 16);
            }
            all0 = v0 != 0; all1 = v1 != 0; uncovered = vu != 0;
            if (uncovered) { if (gl == 0) set_err(err, HIMUT_ERR_COVER); }
            else hap = all0 ? HAP_0 : (all1 ? HAP_1 : HAP_NONE);
        }
    }
    if (gl == 0) H.hap[k] = hap;
}

// ---------------------------------------------------------------------------------------
// k_window_index: per block of 256 reference positions, the range of reads that can
// cover a position of the block (reads are coordinate sorted).
__global__ void __launch_bounds__(256) k_window_index(Reads R, int64_t nblk, int32_t* winlo, int32_t* winhi) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblk) return;
    const int32_t p0 = (int32_t)(b << WIN_SHIFT), p1 = (int32_t)((b + 1) << WIN_SHIFT);
    const int64_t hi = lower_bound(R.tstart, (int64_t)0, R.n, p1);           // reads with tstart < p1
    // a read ending exactly at p0 still belongs: a trailing insertion is counted at tend (caller.py:66-67)
    int64_t lo = lower_bound(R.prefmax_tend, (int64_t)0, hi, p0);            // running max of tend >= p0
    while (lo < hi && R.tend[lo] < p0) lo++;                                 // ... and the first read that really reaches the block
    winlo[b] = (int32_t)lo;
    winhi[b] = (int32_t)hi;
}

__global__ void __launch_bounds__(256) k_count_flags(const uint8_t* flags, int64_t n, unsigned long long* out) {
    unsigned int local = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) local += flags[i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) local += __shfl_down(local, d, 64);
    if ((threadIdx.x & 63) == 0 && local) atomicAdd(out, (unsigned long long)local);
}

}  // namespace himut
