// Read-pass kernels of libhimut_hip.so that more than one pipeline launches (himut_front.hip launches them all):
//
//   k_flag_bases       which reads hold a base outside ATGC (once per pushed batch)
//   k_group_flags      which reads start a group of the decode (once per pushed batch)
//   k_parse_cs         one wave per group of consecutive reads, a wave-parallel tokenizer: cs tag -> gapless segments +
//                      mismatch list + identity (cslib.py:7-64, bamlib.py:47-63); on the call path it also sets the bitmap
//                      of column positions and stores its share of the EMPTY column store
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
// k_parse_cs: a wave-parallel cs tokenizer, one WAVE per group of consecutive reads (k_group_flags).
//
// The text is consumed 1 KB per step, 16 bytes per lane.  Operation starts are the bytes
// ':' '*' '+' '-' '=' (the alternatives of the reference's regex, cslib.py:8; payload bytes
// are digits or letters and can never be one of them), found by every lane in its own 16
// bytes and compacted into an LDS list with one wave scan.  An operation is complete when
// the NEXT start (or the end of the tag) is known, so lane k takes operation k of the
// list: kind = its first byte, payload = the bytes up to the next start.  Reference and
// query offsets are wave prefix sums of the per-operation advances; the mismatch list
// (cslib.py:47-64) and the gapless segments are written at offsets that come from two more
// scans.
//
// Two paths.  decode_read takes one read of any length: only a handful of scalars (running offsets, the open
// aligned run, the unfinished last operation) carry from one step to the next.  decode_group takes the tags of
// several consecutive reads, which lie back to back in R.cs and together fit one step, as ONE text: a tag is 143
// bytes on average, so a wave of its own leaves most lanes of the byte-parallel part and a third of the operation
// round idle, at the same instruction count.  The boundaries between the reads are handled in the lane dimension
// (the comment at decode_group); the wave's running state stays scalar.

constexpr int PB = 1024;  // cs bytes per step

// The group plan (k_group_flags, once per pushed batch; a function of cs_off alone).  Read r starts a group when its
// tag starts in another tile of GROUP_T text bytes than its predecessor's, when it or its predecessor is long (more
// than GROUP_LONG bytes: a group of one), or when it is the 64th, 128th, ... read of its tile.  The tags of a group
// of several reads all start inside one tile and are at most GROUP_LONG bytes each: their text spans at most
// GROUP_T - 1 + GROUP_LONG = PB bytes, one step.
constexpr int GROUP_T = 768;
constexpr int GROUP_LONG = PB - GROUP_T + 1;
constexpr int GROUP_MAX = 64;            // reads of a group: a lane each

// all != 0 (himut_debug_decode, mode 1): every read a group of its own
__global__ void __launch_bounds__(256) k_group_flags(int64_t n, const int64_t* cs_off, int all, uint8_t* flag) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    bool st = true;
    if (!all && r > 0) {
        const int64_t a = cs_off[r - 1], b = cs_off[r], e = cs_off[r + 1];
        const int64_t tile = b / GROUP_T;
        st = a / GROUP_T != tile || e - b > GROUP_LONG || b - a > GROUP_LONG;
        if (!st) st = ((r - lower_bound(cs_off, (int64_t)0, r, tile * GROUP_T)) & (GROUP_MAX - 1)) == 0;   // r - the tile's first read
    }
    flag[r] = st ? 1 : 0;
}

// posbits (call path; else null): the bitmap of reference positions at which a column must be captured = every
// substitution of every read that passes the filters known before the qualities have been streamed (identity,
// mapq, qlen: caller.py:312-317).  A superset of the candidate positions -- the whole-read quality mean
// (caller.py:310), the trim and mismatch-window filters and the chunk rules only take proposals away (propose_read,
// the tail of the capture wave, which knows the mean by then) -- and nearly equal to them.  The wave keeps the
// positions of its reads in LDS and sets the bits once the identity is known (on the per-read path a read with more
// substitutions than the list holds sets them as it goes: a superset is all that is asked for); the atomics cost
// the decode nothing, it is bound by instruction issue.
constexpr int MARK_CAP = 128;

// a wave's LDS.  decode_read: 32 bytes of the previous step and this step's text, the operation starts relative to
// the step (an operation carried over from an earlier step keeps its start in a register), MARK_CAP positions.
constexpr int RL_STARTS = 32 + PB + 32, RL_MARKS = RL_STARTS + 2 * (PB + 8);
// decode_group: the text, the starts (an operation takes two bytes or more: 512 and the end), a bit per text byte
// that is a read's first, seven words per read and one entry behind the last read, the positions of the
// substitutions (three bytes or more each) and their reads
constexpr int GL_STARTS = PB, GL_HEADS = GL_STARTS + 2 * 520, GL_READS = GL_HEADS + 4 * 36, GL_RN = GROUP_MAX + 1;
constexpr int GROUP_MARKS = 344;
constexpr int GL_MPOS = (GL_READS + 7 * 4 * GL_RN + 15) / 16 * 16, GL_MRID = GL_MPOS + 4 * GROUP_MARKS;
constexpr int PARSE_LDS = (GL_MRID + GROUP_MARKS + 15) / 16 * 16;
static_assert(RL_MARKS + 4 * MARK_CAP <= PARSE_LDS, "the per-read path's arrays fit the wave's LDS");

// Operation starts among the first nhere of a lane's 16 text bytes, four bytes at a time in the registers they came
// in: stf gets 0x80 in the bytes that start an operation; returns whether a byte has no place in the reference's
// pattern.  A byte's class comes from two 16-entry tables looked up with v_perm_b32, one by its high nibble (which
// row of the ASCII table), one by its low nibble (which rows that column belongs to): bit 0 / 1 = an operation's
// first byte (* + - in row 2, : = in row 3), bits 2..4 = payload (digits, upper case, lower case)
__device__ __forceinline__ bool cs_classify16(const uint4& v, int nhere, uint32_t stf[4]) {
    const uint32_t words[4] = {v.x, v.y, v.z, v.w};
    bool bad = false;
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
        if (~ok & inside) bad = true;
    }
    return bad;
}

// lanes below this one in the mask
__device__ __forceinline__ int wave_rank_below(unsigned long long b) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// ---- the per-read path: read r of any length, the whole wave.  Groups of one, groups that hold a secondary read,
// and every read of a group in which decode_group met an error.
__device__ __forceinline__ void decode_read(const Reads& R, const Derived& D, const Params& P, const int64_t r, int* err, uint8_t* ccs,
                                            uint32_t* posbits, const int64_t nposwords, uint8_t* mem, const int lane) {
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
    uint8_t* txt = mem;
    uint16_t* starts = reinterpret_cast<uint16_t*>(mem + RL_STARTS);
    Seg* segs = D.segs + sb;
    int32_t* mis = D.mis + sb;
    uint32_t* mq = D.mq + sb;
    const int32_t qlen = uni(R.qlen[r]);
    int32_t* marks = reinterpret_cast<int32_t*>(mem + RL_MARKS);
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
    // the join.
    const int last_base = ((max(n, 1) - 1) / PB) * PB;
    uint4 vcur;
    __builtin_memcpy(&vcur, cs + 16 * lane, 16);                   // himut_push_reads leaves 2 KB of slack behind the text
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
        // ---- operation starts in this lane's 16 bytes
        uint32_t stf[4];                                             // 0x80 in the bytes that start an operation
        if (cs_classify16(v, min(max(nb - 16 * lane, 0), 16), stf)) bad = HIMUT_ERR_CS;   // a byte the reference's pattern has no place for
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

// Does the text of the reads [r0, r0 + G), at most PB bytes, hold a '='?  Long-form tags (minimap2 --cs=long, which himut
// does not ask for) carry RF_LONGCS per read: their groups are taken read by read.  A pass of its own in front of
// decode_group, asked for only in a batch that holds a '=' at all, so that these reads count as planned for the per-read
// path and "taken through it after decode_group gave up" keeps meaning an error.
__device__ __forceinline__ bool long_form_text(const Reads& R, const int64_t r0, const int G, const int lane) {
    const int64_t c0 = uni(R.cs_off[r0]), c1 = uni(R.cs_off[r0 + G]);
    if (c1 - c0 > PB || c1 <= c0) return false;
    uint4 v;
    __builtin_memcpy(&v, R.cs + c0 + 16 * lane, 16);
    const int nhere = min(max((int)(c1 - c0) - 16 * lane, 0), 16);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int nv = min(max(nhere - 4 * k, 0), 4);
        const uint32_t inside = nv >= 4 ? 0x80808080u : (0x80808080u & ((1u << (8 * nv)) - 1u));
        if (cs_eq_bytes(w[k] & 0x7f7f7f7fu, '=') & ~w[k] & inside) any = true;
    }
    return __ballot(any) != 0;
}

// ---- the grouped path: the G reads [r0, r0 + G) of a group, none secondary, as one text of at most PB bytes.
// Returns false, having set no error, flag or bit, when anything is wrong with any of the tags: the caller then
// takes every read of the group through decode_read, which raises what there is to raise.
//
// The lanes i < G are the reads (coalesced loads of their fields); lane = operation in the rounds, as in
// decode_read.  A bit per text byte marks the reads' first bytes, so an operation knows whether it is the head of a
// read, and its read is the count of heads up to it.  All prefix sums run over the whole group: the lane of a head
// operation leaves the prefixes in front of it in LDS under its read, and every operation takes its own values as the
// difference to its read's entry.  A read's totals are the differences between consecutive entries (the last read's:
// to the group's totals).  Three scans do: the reference advance; the mismatch count (indel bases and
// substitutions: at most one per text byte) packed with the deleted bases; the previous indel.  Matches are the
// reference advance less substitutions and deleted bases, the query advance is the reference advance less deleted
// plus inserted bases.  Segment, mismatch and N-substitution ranks are ballots.  The previous-indel logic takes a
// head as a boundary: an indel with none before it in its own read closes a run that starts at (tstart, qstart).
// The read's last operation -- its successor is a head, or it is the group's last -- closes the open run or writes
// the marker segment behind a trailing insertion.  Across rounds the open read's run start, last indel and last kind
// are scalars, as in decode_read.
__device__ __forceinline__ bool decode_group(const Reads& R, const Derived& D, const Params& P, const int64_t r0, const int G, uint8_t* ccs,
                                             uint32_t* posbits, const int64_t nposwords, uint8_t* mem, const int lane) {
    uint8_t* txt = mem;
    uint16_t* starts = reinterpret_cast<uint16_t*>(mem + GL_STARTS);
    uint32_t* headbits = reinterpret_cast<uint32_t*>(mem + GL_HEADS);
    int32_t* s_t0 = reinterpret_cast<int32_t*>(mem + GL_READS);      // tstart; at the end: the read's marks count
    int32_t* s_q0 = s_t0 + GL_RN;                                     // qstart
    int32_t* s_sb = s_q0 + GL_RN;                                     // the read's first slot, relative to the group's
    int32_t* s_ht = s_sb + GL_RN;                                     // in front of the read's head: the reference advance,
    int32_t* s_hx = s_ht + GL_RN;                                     //   mismatches | deleted bases << 16,
    int32_t* s_hsm = s_hx + GL_RN;                                    //   segments | mismatch entries << 16,
    int32_t* s_hnes = s_hsm + GL_RN;                                  //   N substitutions | substitutions << 20
    int32_t* mpos = reinterpret_cast<int32_t*>(mem + GL_MPOS);
    uint8_t* mrid = mem + GL_MRID;

    const int64_t c0 = uni(R.cs_off[r0]), c1 = uni(R.cs_off[r0 + G]);
    if (c1 - c0 > PB || c1 <= c0) return false;                      // (the plan rules the first out)
    const int n = (int)(c1 - c0);
    uint4 v;
    __builtin_memcpy(&v, R.cs + c0 + 16 * lane, 16);                 // both input paths leave 2 KB of slack behind the text
    // ---- the reads
    const bool isread = lane < G;
    const int64_t r = r0 + (isread ? lane : 0);
    const int64_t off = R.cs_off[r], offn = R.cs_off[r + 1];
    const int32_t tstart = R.tstart[r], tend = R.tend[r], qstart = R.qstart[r], qlen = R.qlen[r];
    const int mapq = R.mapq[r];
    const int64_t qoff = R.qoff[r];
    const int h = (int)(off - c0);
    bool bad = isread && offn <= off;                                // an empty tag
    *reinterpret_cast<uint4*>(txt + 16 * lane) = v;
    if (lane < 36) headbits[lane] = 0;
    if (isread) { s_t0[lane] = tstart; s_q0[lane] = qstart; s_sb[lane] = (int)((off >> 1) - (c0 >> 1)) + lane; }
    if (lane == 0) s_sb[G] = (int)((c1 >> 1) - (c0 >> 1)) + G;
    __builtin_amdgcn_wave_barrier();
    if (isread && !bad) {
        atomicOr(&headbits[h >> 5], 1u << (h & 31));
        if (!cs_is_start(txt[h])) bad = true;                        // the tag does not begin with an operation
    }
    // ---- operation starts
    uint32_t stf[4];
    if (cs_classify16(v, min(max(n - 16 * lane, 0), 16), stf)) bad = true;
    const int cnt = __popc(stf[0]) + __popc(stf[1]) + __popc(stf[2]) + __popc(stf[3]);
    const int incl = wave_incl_add(cnt, lane);
    const int nops = lane_val(incl, 63);
    if (__ballot(bad) || nops > 512) return false;                   // (more starts than half the bytes: an operation without payload)
    {
        int w = incl - cnt;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t mk = stf[k];
            while (mk) { const int i = __ffs((int)mk) - 1; mk &= mk - 1; starts[w++] = (uint16_t)(16 * lane + 4 * k + (i >> 3)); }
        }
    }
    if (lane == 0) starts[nops] = (uint16_t)n;
    __builtin_amdgcn_wave_barrier();
    // (the first read's head is byte 0, an operation start: operation 0 is a head)
    const int64_t sb0 = (c0 >> 1) + r0;
    // wave-uniform running state: the group's totals so far, the heads so far, the open read's run
    int Tg = 0, Xg = 0, NS = 0, NM = 0, NN = 0, NB = 0, rbase = 0, nmark = 0;
    int last_kind = 0, run_t0 = 0, run_q0 = 0; bool run_ins = false;
    for (int k0 = 0; k0 < nops; k0 += 64) {
        const int k = k0 + lane;
        const bool valid = k < nops;
        int s = 0, e = 0, kind = 0, len = 0, dt = 0, ref = 0, alt = 0;
        bool head = false, is_last = false;
        if (valid) {
            s = (int)starts[k]; e = (int)starts[k + 1];
            kind = (int)txt[s];
            len = e - s - 1;
            head = (headbits[s >> 5] >> (s & 31)) & 1u;
            is_last = k + 1 == nops || ((headbits[e >> 5] >> (e & 31)) & 1u);
            if (kind == ':') {
                if (len < 1 || len > 9) bad = true;
                else {
                    int x = 0;
                    for (int i = 0; i < len; i++) {
                        const int c = txt[s + 1 + i];
                        if (!cs_is_digit(c)) bad = true;
                        x = x * 10 + (c - '0');
                    }
                    dt = x;
                }
            } else if (kind == '*') {
                const int a = txt[s + 1], b = (len >= 2) ? (int)txt[s + 2] : 0;
                if (len != 2 || !(a >= 'a' && a <= 'z') || !(b >= 'a' && b <= 'z')) bad = true;   // \*[a-z][a-z]
                ref = a - 32; alt = b - 32;
                dt = 1;
            } else {
                if (len < 1) bad = true;
                if (kind != '+') dt = len;
            }
        }
        if (__ballot(bad)) return false;                             // before anything is written: ranks of a malformed text prove nothing
        const bool indel = valid && (kind == '+' || kind == '-'), isdel = valid && kind == '-';
        const bool sub = valid && kind == '*';
        const int dq = isdel ? 0 : (indel ? len : dt);
        // ---- what depends on the kinds alone: the ranks
        int prev_kind = __shfl_up(kind, 1, 64);
        if (lane == 0) prev_kind = last_kind;
        if (head) prev_kind = 0;
        const bool run_before = indel && prev_kind != 0 && prev_kind != '+' && prev_kind != '-';   // an indel closes the aligned run before it
        const bool endseg = is_last && (!indel || kind == '+');      // the read's open run, or the marker behind a trailing insertion
        const int nseg_here = (run_before ? 1 : 0) + (isdel ? 1 : 0) + (endseg ? 1 : 0);   // two at the most
        const bool ismis = indel || (sub && ref != 'N'), nsb = sub && ref == 'N';
        const unsigned long long hb = __ballot(head);
        const int rid = rbase + wave_rank_below(hb) + (head ? 1 : 0) - 1;
        const unsigned long long hle = hb & (~0ull >> (63 - lane));
        const int hl = hle ? 63 - __clzll((long long)hle) : -1;     // the lane of this operation's head (-1: an earlier round)
        const int x = (sub ? 1 : (indel ? len : 0)) | ((isdel ? len : 0) << 16);
        const int it = wave_incl_add(dt, lane), ix = wave_incl_add(x, lane);
        const int iseg = wave_rank_incl(nseg_here >= 1) + wave_rank_incl(nseg_here == 2), imis = wave_rank_incl(ismis);
        const int inn = wave_rank_incl(nsb), isb = wave_rank_incl(sub);
        // the group's prefixes in front of this operation
        const int gtb = Tg + it - dt, pxb = Xg + ix - x;
        const int segb = NS + iseg - nseg_here, misb = NM + imis - (ismis ? 1 : 0);
        const int nnb = NN + inn - (nsb ? 1 : 0), sbb = NB + isb - (sub ? 1 : 0);
        if (head) { s_ht[rid] = gtb; s_hx[rid] = pxb; s_hsm[rid] = segb | (misb << 16); s_hnes[rid] = nnb | (sbb << 20); }
        __builtin_amdgcn_wave_barrier();
        int t0r = 0, q0r = 0, sbr = 0, htr = 0, hxr = 0, hsmr = 0, hnesr = 0;
        if (valid) { t0r = s_t0[rid]; q0r = s_q0[rid]; sbr = s_sb[rid]; htr = s_ht[rid]; hxr = s_hx[rid]; hsmr = s_hsm[rid]; hnesr = s_hnes[rid]; }
        // ---- reference / query offset at the operation and after it
        const int adv = gtb - htr;
        const int tk = t0r + adv;
        const int qk = q0r + adv - 2 * ((pxb >> 16) - (hxr >> 16)) + ((pxb & 0xffff) - (hxr & 0xffff)) - (sbb - (hnesr >> 20));
        const int ta = tk + dt, qa = qk + dq;
        // the previous indel of the operation's own read
        const int pidx = wave_incl_max(indel ? lane : -1, lane);
        int Pk = __shfl_up(pidx, 1, 64);
        if (lane == 0) Pk = -1;
        const bool have_p = Pk >= 0 && Pk >= hl;
        const int src = have_p ? Pk : 0;
        const int p_ta = __shfl(ta, src, 64), p_qa = __shfl(qa, src, 64), p_kind = __shfl(kind, src, 64);
        // the aligned run that holds or ends in front of this operation: behind that indel, else from the read's start
        const int rt0 = have_p ? p_ta : (hl >= 0 ? t0r : run_t0), rq0 = have_p ? p_qa : (hl >= 0 ? q0r : run_q0);
        const bool rins = have_p ? p_kind == '+' : (hl >= 0 ? false : run_ins);
        const int64_t sb = sb0 + sbr;
        if (nseg_here) {
            Seg* w = D.segs + sb + (segb - (hsmr & 0xffff));
            if (run_before) { const Seg z = {rt0, rq0, tk - rt0, rins ? SEG_INS : 0u}; *w++ = z; }
            if (isdel) { const Seg z = {tk, qk, len, SEG_DEL | (prev_kind == '+' ? SEG_INS : 0u)}; *w++ = z; }   // a deletion is a segment of its own
            if (endseg) { const Seg z = {indel ? ta : rt0, indel ? qa : rq0, indel ? 0 : ta - rt0, (indel || rins) ? SEG_INS : 0u}; *w = z; }
        }
        // mismatch list (cslib.py:54-62): substitutions with a non-N reference base, all indels
        int aa = 0, ra = 0, seq_nib = -1;
        if (sub) {
            aa = char2allele(alt);
            if (aa < 0) bad = true;                                  // caller.py:62
            if (ref != 'N') { ra = char2allele(ref); if (ra < 0) bad = true; }   // bamlib.py:188
            if (ref != 'N' && !bad) {                                // the base cs names must be the base SEQ holds
                if (qk < 0 || qk >= R.qlen[r0 + rid]) bad = true;
                else seq_nib = nib_at(R.seq, R.qoff[r0 + rid] + qk);
            }
        }
        if (ismis) {
            const int64_t w = sb + (misb - (hsmr >> 16));
            D.mis[w] = tk + 1;
            D.mq[w] = sub ? (((uint32_t)qk << 5) | 16u | ((uint32_t)(ra & 3) << 2) | (uint32_t)(aa & 3)) : ((uint32_t)qk << 5);
        }
        if (nsb) {                                                   // no mismatch entry, but normcounts counts its base: from the top of the read's slots
            const int top = s_sb[rid + 1] - sbr - 1;
            D.mq[sb + top - (nnb - (hnesr & 0x3ff))] = ((uint32_t)qk << 5) | 8u;
        }
        if (posbits) {
            const bool mk = sub && ref != 'N';
            const unsigned long long mb = __ballot(mk);
            if (mk) { const int i = nmark + wave_rank_below(mb); mpos[i] = tk; mrid[i] = (uint8_t)rid; }
            nmark += __popcll(mb);
        }
        // ---- carry the round's end state
        const int ll = min(64, nops - k0) - 1;                       // the round's last operation
        Tg += lane_val(it, 63); Xg += lane_val(ix, 63);
        NS += lane_val(iseg, 63); NM += lane_val(imis, 63); NN += lane_val(inn, 63); NB += lane_val(isb, 63);
        rbase += __popcll(hb);
        const int Lh = lane_val(hl, ll), Li = lane_val(pidx, ll);
        if (Li >= 0 && Li >= Lh) { run_t0 = lane_val(ta, Li); run_q0 = lane_val(qa, Li); run_ins = lane_val(kind, Li) == '+'; }
        else if (Lh >= 0) { run_t0 = lane_val(t0r, ll); run_q0 = lane_val(q0r, ll); run_ins = false; }
        last_kind = lane_val(kind, ll);
        if (seq_nib >= 0 && nib2allele(seq_nib) != aa) bad = true;   // the substitutions' bases against SEQ
        if (__ballot(bad)) return false;
    }
    // ---- the reads' totals: differences between consecutive heads
    if (lane == 0) { s_ht[G] = Tg; s_hx[G] = Xg; s_hsm[G] = NS | (NM << 16); s_hnes[G] = NN | (NB << 20); }
    __builtin_amdgcn_wave_barrier();
    int ns = 0, nm = 0, nN = 0, match = 0, mism = 0;
    if (isread) {
        const int dT = s_ht[lane + 1] - s_ht[lane];
        const int xa = s_hx[lane], xb = s_hx[lane + 1], ma = s_hsm[lane], mb = s_hsm[lane + 1], na = s_hnes[lane], nb = s_hnes[lane + 1];
        const int dDL = (xb >> 16) - (xa >> 16), dS = (nb >> 20) - (na >> 20);
        mism = (xb & 0xffff) - (xa & 0xffff);
        match = dT - dS - dDL;
        ns = (mb & 0xffff) - (ma & 0xffff); nm = (mb >> 16) - (ma >> 16);
        nN = (nb & 0x3ff) - (na & 0x3ff);
        const int t = tstart + dT, q = qstart + dT - 2 * dDL + mism - dS;
        if (t != tend || q > qlen) bad = true;                       // cs inconsistent with CIGAR / SEQ
        if ((long long)match + (long long)mism == 0) bad = true;     // ZeroDivisionError in the reference (bamlib.py:62)
    }
    if (__ballot(bad)) return false;
    if (isread) {
        // identity filter (bamlib.py:47-63, caller.py:314); the other read filters follow behind the capture
        const long long match_all = (long long)match, mism_all = (long long)mism;
        const double ident = (double)match_all / (double)(match_all + mism_all);
        const bool ident_ok = !(ident < P.p.min_sequence_identity);
        const uint8_t fl = ident_ok ? RF_IDENT_OK : 0;    // (no RF_LONGCS: long_form_text keeps such a group off this path)
        ReadMeta M;
        M.tstart = tstart; M.tend = tend; M.nseg = ns; M.flags = fl; M.segbase = (off >> 1) + r; M.qoff = qoff;
        D.nseg[r] = ns; D.nmis[r] = nm; D.nnsub[r] = nN; D.rflag[r] = fl; D.meta[r] = M;
        ccs[r] = 0;                          // the flag propose_read raises for a read that may propose (num_ccs)
        s_t0[lane] = (ident_ok && !(mapq < P.p.min_mapq) && (P.p.qlen_lower_limit < qlen && qlen < P.p.qlen_upper_limit)) ? 1 : 0;   // caller.py:312-317
    }
    if (nmark > 0) {                         // the substitutions of the reads that pass, into the bitmap
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < nmark; i += 64) {
            const int32_t p = mpos[i];
            if (s_t0[mrid[i]] && p >= 0 && (int64_t)(p >> 5) < nposwords) atomicOr(posbits + (p >> 5), 1u << (p & 31));
        }
    }
    return true;
}

// What limits the waves of this kernel is LDS and the scalar registers (the values the wave keeps uniform).  The
// grouped path's arrays take 23,040 B per workgroup: 7 workgroups per CU.  256-thread workgroups are admitted per CU up
// to 800 / (ceil(sgpr / 16) * 16 + 16) (MI355X_MICROARCH.md): a cap of 96 scalars admits the same 7 (the compiler takes 94
// under it, with spills to vector lanes and no scratch); the 80 that gave the one-path kernel 8 workgroups would buy
// nothing here, and the 106 the compiler takes unasked give 6.
#ifndef HIMUT_PARSE_SGPR
#define HIMUT_PARSE_SGPR 96
#endif
// gfirst[g]: the first read of group g of ngroups (the plan); longcs: the batch holds a '=' somewhere (the host knows from
// the push or the ingest: only then is a group's text looked through for one); dbg (tests; else null): counts groups, groups of several
// reads, reads planned for the per-read path, reads taken through it after decode_group gave up.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(HIMUT_PARSE_SGPR)))
k_parse_cs(Reads R, Derived D, Params P, int* err, uint8_t* ccs, uint32_t* posbits, int64_t nposwords, uint4* fill, int64_t fill16,
           int fill_per, const int32_t* gfirst, int64_t ngroups, int longcs, unsigned long long* dbg) {
    __shared__ __align__(16) uint8_t s_mem[4][PARSE_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wv = uni(tid >> 6);
    const int64_t g = (int64_t)blockIdx.x * 4 + wv;
    if (g >= ngroups) return;
    // The column store must be EMPTY before the capture writes into it (fill: its fill16 16-byte pieces, or null).  The
    // decode leaves the memory system idle: every wave stores its share, fill_per pieces per lane, and neither a fill
    // between the decode and the capture nor a second stream is needed.
    if (fill) {
        const uint4 e = make_uint4(0x00070007u, 0x00070007u, 0x00070007u, 0x00070007u);   // CELL_EMPTY
        const int64_t f0 = g * 64 * fill_per;
        for (int k = 0; k < fill_per; k++) { const int64_t o = f0 + 64 * k + lane; if (o < fill16) fill[o] = e; }
    }
    const int64_t r0 = uni(gfirst[g]), r1 = g + 1 < ngroups ? (int64_t)uni(gfirst[g + 1]) : R.n;
    const int G = (int)(r1 - r0);
    uint8_t* mem = s_mem[wv];
    bool grouped = G > 1 && G <= GROUP_MAX;
    if (grouped && __ballot(lane < G && (R.flag[r0 + (lane < G ? lane : 0)] & 0x100))) grouped = false;   // a secondary read: bamlib.py:17
    if (grouped && longcs && long_form_text(R, r0, G, lane)) grouped = false;
    int redone = 0;
    if (grouped && !decode_group(R, D, P, r0, G, ccs, posbits, nposwords, mem, lane)) { grouped = false; redone = G; }
    if (!grouped) {
        for (int64_t r = r0; r < r1; r++) {
            __builtin_amdgcn_wave_barrier();
            decode_read(R, D, P, r, err, ccs, posbits, nposwords, mem, lane);
        }
    }
    if (dbg && lane == 0) {
        atomicAdd(dbg, 1ull);
        if (G > 1) atomicAdd(dbg + 1, 1ull);
        if (!grouped && !redone) atomicAdd(dbg + 2, (unsigned long long)G);
        if (redone) atomicAdd(dbg + 3, (unsigned long long)redone);
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
