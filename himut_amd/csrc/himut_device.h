// Types, constants and __device__ helpers that more than one pipeline of libhimut_hip.so uses: the read batch and
// what the cs decode derives from it, the chunk tables, the phase sets, the run parameters, the genotype LUT, the
// site sets, the column index.  No kernels: each __global__ lives in the header of the one source file that
// launches it (himut_reads.h, himut_front.h, himut_call.h, himut_pile.h, himut_norm.h / himut_normq.h, himut_ingest.h, himut_fasta.h,
// himut_edges.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "himut_hip.h"

namespace himut {

constexpr int WIN_SHIFT = 8;  // k_window_index granularity: 256 reference positions
constexpr int CHUNK_HINT_SHIFT = 14;  // chunk look-up hint granularity: 16 kb

// k_pile_dense geometry: tile width, LDS row batch, threads
constexpr int PD_TP = 512, PD_RB = 56, PD_NT = 256;

// pile cell: bits 0-2 allele, bit 3 "an insertion precedes this position"
constexpr uint8_t CELL_OTHER = 4;  // query base outside ATGC (reference raises KeyError)
constexpr uint8_t CELL_DEL = 5;
constexpr uint8_t CELL_EMPTY = 7;
constexpr uint8_t CELL_INS = 8;

constexpr uint32_t SEG_DEL = 1;
constexpr uint32_t SEG_INS = 2;

constexpr uint8_t RF_SECONDARY = 1;
constexpr uint8_t RF_PASS = 2;
constexpr uint8_t RF_IDENT_OK = 4;
constexpr uint8_t RF_LONGCS = 8;

constexpr uint8_t REC_GERM = 1;        // dropped as germline (caller.py:338-345): counted, no record
constexpr uint8_t REC_SUPPRESSED = 2;  // tpos already in som_seen from an earlier chunk
constexpr uint8_t REC_DUP = 4;         // identical tuple (HetAltSite printed once)

constexpr uint8_t HAP_0 = 0, HAP_1 = 1, HAP_NONE = 2;

struct Seg {
    int32_t t0;      // first reference position (0-based)
    int32_t q0;      // query offset of the first base (soft clip included)
    int32_t len;     // reference length (0 for a trailing insertion marker)
    uint32_t flags;  // SEG_DEL | SEG_INS
};

struct Reads {
    int64_t n;
    const int32_t *tstart, *tend, *qstart, *qlen;
    const uint8_t* mapq;
    const uint16_t* flag;
    const int32_t* qid;
    const int64_t *qoff, *cs_off;
    const uint8_t *seq, *bq, *cs;
    const int32_t* prefmax_tend;  // running maximum of tend in file order
    const uint8_t* nonacgt;       // per read: SEQ holds a base outside ATGC somewhere (k_flag_bases, once per pushed batch)
};

struct Derived {
    uint32_t* bqsum;
    int32_t* nseg;
    int32_t* nmis;
    Seg* segs;       // seg_base(r) = (cs_off[r] >> 1) + r
    int32_t* mis;    // same base; 1-based mismatch positions (cslib.py:54-62)
    uint32_t* mq;    // same base; per mismatch: qpos << 5 | (substitution ? 16 | ref << 2 | alt : 0)
    uint8_t* rflag;
    struct ReadMeta* meta;
    int32_t* nnsub;  // substitutions whose reference base is N (cslib.py:54-56 keeps them out of the mismatch list): their
                     // query offsets sit in mq[] from the TOP of the read's slots downwards, mq[top - k] = qpos << 5 | 8
};

// everything a pile row needs about its read, in one 32-byte load
struct ReadMeta {
    int32_t tstart, tend;
    int32_t nseg;
    uint32_t flags;   // RF_*
    int64_t segbase;
    int64_t qoff;
};

// one chunk, in the order of the sorted starts
struct ChunkRec {
    int32_t start, end;
    int32_t idx;        // chunk index
    int32_t pmaxend;    // running maximum of end up to and including this one
    int64_t maskoff;    // first mask cell
    int64_t pairbase;   // pairoff - rlo: + read index = the (chunk, read) pair
};

// what k_mask_emit needs about a mask tile (MASK_TILE_CELLS cells): the chunk of its first cell
struct MaskTile {
    int32_t ck0;      // chunk of the tile's first cell
    int32_t start0;   // its start
    int64_t off0;     // its first cell
    int64_t off1;     // first cell of the next chunk
    int64_t pad;
};
constexpr int MASK_TILE_SHIFT = 13;
constexpr int MASK_TILE_CELLS = 1 << MASK_TILE_SHIFT;

struct Chunks {
    int64_t n;
    const ChunkRec* rec;       // sorted by start
    const MaskTile* mtile;     // per mask tile
    const int32_t *start, *end;
    const int64_t* maskoff;    // prefix of (end - start + 1)
    const int32_t* s_start;    // starts sorted ascending
    const int32_t* s_idx;      // chunk index per sorted slot
    const int32_t* s_pmaxend;  // prefix maximum of end in sorted order
    const int64_t* rlo;        // first read with prefmax_tend > start
    const int64_t* rhi;        // first read with tstart >= end
    const int64_t* pairoff;    // prefix of (rhi - rlo)
    const int32_t* hint;       // hint[p >> CHUNK_HINT_SHIFT] = number of sorted starts <= (p >> SHIFT) << SHIFT
    int64_t nhint;
};

struct Phase {
    const int64_t* off;
    const int32_t* hpos;
    const uint8_t *href, *halt, *hbit;
    uint8_t* hap;  // per (chunk, read) pair
};

struct Params {
    himut_params p;
    int32_t unique_qnames;
};

struct GtLut {
    double t[3][256];  // hom / het / err indexed by BQ
    double prior[4];   // homref het hetalt homalt
};

// one proposed (chunk, tpos, ref, alt)
struct Cand {
    int32_t tpos;        // 1-based
    uint32_t chunk_bit;  // chunk << 4 | (ref << 2 | alt)
};

__device__ __forceinline__ int64_t seg_base(const Reads& R, int64_t r) { return (R.cs_off[r] >> 1) + r; }

__device__ __forceinline__ int nib_at(const uint8_t* seq, int64_t o) {
    uint8_t b = seq[o >> 1];
    return (o & 1) ? (b & 15) : (b >> 4);
}
// BAM nibble -> himut allele index A0 T1 G2 C3 (util.py:14-20), 4 otherwise
__device__ __forceinline__ int nib2allele(int n) { return (int)((0x4444444144424304ULL >> (4 * n)) & 15); }
__device__ __forceinline__ int nib2char(int n) { return "=ACMGRSVTWYHKDBN"[n]; }
__device__ __forceinline__ int allele2char(int a) { return (int)((0x43475441u >> (8 * (a & 3))) & 255); }  // "ATGC"
__device__ __forceinline__ int char2allele(int c) {
    return c == 'A' ? 0 : c == 'T' ? 1 : c == 'G' ? 2 : c == 'C' ? 3 : -1;
}
__device__ __forceinline__ int asc_rank(int a) { return a == 0 ? 0 : a == 3 ? 1 : a == 2 ? 2 : 3; }  // A<C<G<T
__device__ __forceinline__ int upper(int c) { return (c >= 'a' && c <= 'z') ? c - 32 : c; }
__device__ __forceinline__ bool is_alpha(int c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }

// every aligned base of read r (the gapless segments that are not deletions) is one of ATGC?  For the lanes [l0, l0 + nl) of
// a wave together; the answer is valid in every one of them.  (A flagged read only: k_flag_bases.)
__device__ __forceinline__ bool aligned_bases_ok(const Reads& R, const Seg* segs, int ns, int64_t qo, int l, int nl) {
    bool ok = true;
    for (int j = 0; j < ns; j++) {
        const Seg g = segs[j];
        if ((g.flags & SEG_DEL) || g.len <= 0) continue;
        for (int32_t i = l; i < g.len; i += nl) if (nib2allele(nib_at(R.seq, qo + g.q0 + i)) > 3) ok = false;
    }
    return ok;
}

// 16 BAM nibbles (base j at bits 4j..4j+3) -> 16 pile cells (himut allele index, 4 = not ATGC)
__device__ __forceinline__ uint64_t nib16_to_cells(uint64_t x) {
    const uint64_t m = 0x1111111111111111ULL;
    const uint64_t n0 = x & m, n1 = (x >> 1) & m, n2 = (x >> 2) & m, n3 = (x >> 3) & m;  // A C G T one-hot bits
    const uint64_t sum = n0 + n1 + n2 + n3;
    const uint64_t inv = ((sum >> 1) | (sum >> 2) | ~sum) & m;     // not exactly one bit set
    uint64_t code = (n3 | n1) | ((n2 | n1) << 1);                  // T,C -> bit0 ; G,C -> bit1
    code = (code & ~(inv * 3)) | (inv << 2);
    return code;
}

// XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs, so give
// each XCD a contiguous range of tiles (neighbouring tiles share reads and
// metadata -> same L2).  Bijective for any n (speed only, never correctness).
__device__ __forceinline__ int64_t xcd_remap(int64_t b, int64_t n) {
    const int64_t q = n >> 3, rm = n & 7, x = b & 7;
    const int64_t base = x < rm ? x * (q + 1) : rm * (q + 1) + (x - rm) * q;
    return base + (b >> 3);
}

template <class T>
__device__ __forceinline__ int64_t lower_bound(const T* a, int64_t lo, int64_t hi, T x) {  // first a[i] >= x
    while (lo < hi) { int64_t m = (lo + hi) >> 1; if (a[m] < x) lo = m + 1; else hi = m; }
    return lo;
}
template <class T>
__device__ __forceinline__ int64_t upper_bound(const T* a, int64_t lo, int64_t hi, T x) {  // first a[i] > x
    while (lo < hi) { int64_t m = (lo + hi) >> 1; if (x < a[m]) hi = m; else lo = m + 1; }
    return lo;
}

// bamlib.get_mismatch_range (bamlib.py:245-258): the window [s, e] of 1-based reference positions around tpos
__device__ __forceinline__ void mismatch_range(int64_t tpos, int64_t qpos, int64_t qlen, int64_t w, int64_t& s, int64_t& e) {
    const int64_t qs = qpos - w, qe = qpos + w;
    int64_t ur, dr;
    if (qs < 0) { ur = w + qs; dr = w - qs; }
    else if (qe > qlen) { ur = w + (qe - qlen); dr = qlen - qpos; }
    else { ur = w; dr = w; }
    s = tpos - ur; e = tpos + dr;
}

// entries of a read's ascending mismatch list (nm 1-based positions) inside the window [s, e]: bisect_right(e) -
// bisect_left(s).  The positions are int32: a window that begins or ends outside that range is cut to it.
__device__ __forceinline__ int mismatches_in(const int32_t* mis, int nm, int64_t s, int64_t e) {
    const int32_t s32 = (int32_t)max(s, (int64_t)INT32_MIN), e32 = (int32_t)min(e, (int64_t)INT32_MAX);
    return (s > e || s > INT32_MAX || e < INT32_MIN) ? 0 : (int)(upper_bound(mis, (int64_t)0, (int64_t)nm, e32) - lower_bound(mis, (int64_t)0, (int64_t)nm, s32));
}

__device__ __forceinline__ void set_err(int* err, int code) { atomicOr(err, 1 << code); }

// wave-uniform values belong in scalar registers: everything computed from them then runs on the scalar unit
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ int64_t uni(int64_t v) {
    return ((int64_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
// value of lane l, l wave-uniform
__device__ __forceinline__ int lane_val(int v, int l) { return __builtin_amdgcn_readlane(v, l); }

// slot reservation for the lanes that reach this point together: one atomic per wave
__device__ __forceinline__ unsigned long long wave_reserve(unsigned long long* counter) {
    const unsigned long long act = __ballot(1);
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)act) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(act));
    base = __shfl(base, leader, 64);
    return base + (unsigned long long)__popcll(act & ((1ULL << lane) - 1ULL));
}

// inclusive wave scans on the DPP network: four shifts inside each row of 16 lanes, then
// the row totals are carried across with the two row broadcasts
__device__ __forceinline__ int wave_incl_add(int v, int) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast:31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ int wave_incl_max(int v, int) {
    constexpr int lowest = -0x7fffffff - 1;
    v = max(v, __builtin_amdgcn_update_dpp(lowest, v, 0x111, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(lowest, v, 0x112, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(lowest, v, 0x114, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(lowest, v, 0x118, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(lowest, v, 0x142, 0xa, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(lowest, v, 0x143, 0xc, 0xf, false));
    return v;
}
// sum of the n quality bytes at q (16-byte aligned, padded to a multiple of 32), by the whole wave; valid in every lane
// (the support and duplex runs: a read's quality sum where no capture has left one)
__device__ __forceinline__ uint32_t wave_bq_sum(const uint8_t* q, int32_t n, int lane) {
    uint32_t sum = 0;
    for (int32_t o = lane * 16; o < n; o += 1024) {
        const uint4 v = *reinterpret_cast<const uint4*>(q + o);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int rem = n - (o + 4 * k);                 // bytes of the word inside the read
            uint32_t x = w[k];
            if (rem < 4) x = rem <= 0 ? 0u : (x & (0xffffffffu >> (8 * (4 - rem))));
            sum = __builtin_amdgcn_sad_u8(x, 0u, sum);
        }
    }
    return (uint32_t)lane_val(wave_incl_add((int)sum, lane), 63);
}
// inclusive count of the lanes up to and including this one for which p holds
__device__ __forceinline__ int wave_rank_incl(bool p) {
    const unsigned long long b = __ballot(p);
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u)) + (p ? 1 : 0);
}
__device__ __forceinline__ bool cs_is_start(int c) { return c == ':' || c == '*' || c == '+' || c == '-' || c == '='; }
__device__ __forceinline__ bool cs_is_digit(int c) { return c >= '0' && c <= '9'; }
// byte-parallel classification of four ASCII bytes; results carry 0x80 in the bytes that qualify
__device__ __forceinline__ uint32_t cs_eq_bytes(uint32_t w, uint32_t c) {          // bytes equal to c (bytes < 0x80)
    return ~((w ^ (c * 0x01010101u)) + 0x7f7f7f7fu) & 0x80808080u;
}
__device__ __forceinline__ uint32_t cs_ge_bytes(uint32_t w, uint32_t c) {          // bytes >= c (bytes < 0x80, c >= 1)
    return (w + (0x80u - c) * 0x01010101u) & 0x80808080u;
}
__device__ __forceinline__ uint32_t cs_start_bytes(uint32_t w) {
    return cs_eq_bytes(w, ':') | cs_eq_bytes(w, '*') | cs_eq_bytes(w, '+') | cs_eq_bytes(w, '-') | cs_eq_bytes(w, '=');
}
__device__ __forceinline__ uint32_t cs_payload_bytes(uint32_t w) {                 // digits and letters
    return (cs_ge_bytes(w, '0') & ~cs_ge_bytes(w, '9' + 1)) | (cs_ge_bytes(w, 'A') & ~cs_ge_bytes(w, 'Z' + 1)) |
           (cs_ge_bytes(w, 'a') & ~cs_ge_bytes(w, 'z' + 1));
}
__device__ __forceinline__ uint32_t cs_pack4(uint32_t f) {                         // 0x80 flags of bytes 0..3 -> bits 0..3
    const uint32_t g = f >> 7;
    return (g | (g >> 7) | (g >> 14) | (g >> 21)) & 15u;
}

// ---------------------------------------------------------------------------------------
// The column store.  Candidate columns live at the UNIQUE reference positions that carry
// a candidate (several chunks / alts can share one).  All positions of a 256-position block
// share one read window [lo, lo + n) (k_window_index), so a block with cnt candidate
// positions owns n * cnt slots, read-major: the slot of (read r, unique position u) is
// boff[b] + (r - lo) * cnt + (u - ufirst[b]).  Neighbouring positions of one read are
// neighbours in memory, which is what lets the dense sweep read its columns coalesced.
// One 16-bit slot per (read of the window, position), walked in fetch order:
//   bits 0-2 cell (0-3 allele A T G C, 4 base outside ATGC, 5 deletion, 7 not in the pile)
//   bit 3    an insertion precedes the position
//   bit 4    unused
//   bits 8-15 base quality
// k_stream_capture fills it while streaming every read once with coalesced loads;
// walk_column (himut_column.h) consumes it, one thread per column.

struct BlockTab {     // one per 256 reference positions
    int32_t lo;       // first read of the window
    uint32_t ncnt;    // bits 0-21: reads in the window = slots per column; bits 22-31: candidate positions in the block
    uint32_t boff;    // slot offset of the block's first column
    uint32_t ufirst;  // unique-position rank of the block's first candidate position
};
constexpr uint32_t BT_N_MASK = (1u << 22) - 1u;

struct PosIndex {
    const uint32_t* bits;    // bit rpos set: some candidate sits at rpos
    const uint32_t* rank;    // exclusive prefix popcount per 32-bit word, nwords + 1 entries
    int64_t nwords;
    const BlockTab* bt;
    int64_t nblk;
};

// Rank of a position among the column positions = the block's first rank (BlockTab) + the set bits of the block's
// eight bitmap words in front of it (one 32-byte sector).
__device__ __forceinline__ uint32_t pos_rank_in_block(const uint32_t* bits, int32_t rpos) {
    const uint4* wp = reinterpret_cast<const uint4*>(bits + (((int64_t)rpos >> 8) << 3));
    const uint4 a = wp[0], b = wp[1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const int wi = (rpos >> 5) & 7;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t m = k < wi ? 0xffffffffu : (k == wi ? ((1u << (rpos & 31)) - 1u) : 0u);
        c += (uint32_t)__popc(w[k] & m);
    }
    return c;
}
__device__ __forceinline__ uint32_t pos_rank(const PosIndex& X, int32_t rpos) {
    return X.bt[rpos >> 8].ufirst + pos_rank_in_block(X.bits, rpos);
}

struct SiteSets {
    const uint64_t* pon; int64_t npon;
    const uint64_t* com; int64_t ncom;
    const uint32_t* posbits;  // bit tpos set when either set holds a key at that position
    int64_t nposbits;         // number of valid bits
};

__device__ __forceinline__ bool key_in(const uint64_t* a, int64_t n, uint64_t x) {
    int64_t k = lower_bound(a, (int64_t)0, n, x);
    return k < n && a[k] == x;
}

// genotype list of gtlib.py:9 in himut allele indices (A0 T1 G2 C3):
// AA TA CA GA TT CT GT CC GC GG
#define HIMUT_GT_B1(g) ((0x2232312310ULL >> (4 * (g))) & 15)
#define HIMUT_GT_B2(g) ((0x2331110000ULL >> (4 * (g))) & 15)

__device__ __forceinline__ int gt_state_of(int b1, int b2, int ref) {  // gtlib.py:23-38
    if (b1 == b2 && b2 == ref) return 0;
    if ((b1 == ref) != (b2 == ref)) return 1;
    if (b1 != b2) return 2;
    return 3;
}

// A column's three tables' sums per allele, S[table][allele] (gtlib.py:84-93).  A struct, not a bare local array: a bare
// array that the inlined genotype() reads becomes one vector register tuple, which costs the kernels registers; the
// struct's twelve sums stay separate scalars.
struct GtSums {
    double v[3][4];
    __device__ __forceinline__ double* operator[](int t) { return v[t]; }
    __device__ __forceinline__ const double* operator[](int t) const { return v[t]; }
};

// Ten PLs in genotype-list order (gtlib.py:72-110); np.argsort with the scalar insertion sort: ties -> lower index
// (gtlib.py:113-119).  best: the genotype, gq: the gap to the second smallest PL, capped at 99.
struct Genotype { int best, gq; };
__device__ __forceinline__ Genotype genotype(const GtSums& S, const double* prior, int ref) {
    double best = 0.0, second = 0.0;
    int ibest = 0;
#pragma unroll
    for (int g = 0; g < 10; g++) {
        const int b1 = (int)HIMUT_GT_B1(g), b2 = (int)HIMUT_GT_B2(g);
        double acc = 0.0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            double term;
            if (b1 == b2 && b == b1) term = S[0][b];
            else if (b1 != b2 && (b == b1 || b == b2)) term = S[1][b];
            else term = S[2][b];
            acc = acc + term;
        }
        acc = acc + prior[gt_state_of(b1, b2, ref)];
        const double pl = -10.0 * acc;
        if (g == 0) { best = pl; ibest = 0; }
        else if (pl < best) { second = best; best = pl; ibest = g; }
        else if (g == 1 || pl < second) second = pl;
    }
    const double gqf = second - best;
    return {ibest, gqf < 99.0 ? (int)gqf : 99};
}

}  // namespace himut
