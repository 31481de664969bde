// Device code of the column front: what the call, germline, dbs and sites runs have in common between the read pass
// (himut_reads.h: k_parse_cs sets the bitmap of column positions and stores its share of the EMPTY column store) and
// their own kernels.  front_capture (himut_front.hip) launches them in order; DESIGN.md sections 2-4.
//
//   k_block_sums / k_block_table3
//                      per 256-position block the number of column positions and of column-store slots, their
//                      prefix sums (first rank, slot offset) and the block table
//   k_stream_capture   one wave per read, a software pipeline over windows of 2048 query bases: streams the read's
//                      qualities and packed bases once (16-byte coalesced loads, two windows ahead), sums the
//                      qualities (np.mean of the whole query, bamlib.py:34-36), enumerates the column positions
//                      under each window from the bitmap, one per lane, and drops their (allele, BQ) cells into the
//                      column store; then, on the call path, the read's proposals (propose_read): read filters of
//                      caller.py:310-317, trim / mismatch-window filters (bamlib.py:69-86,222-282); every surviving
//                      (chunk, tpos, ref, alt) sets its bit in a per-chunk mask (the set() of caller.py:324), from
//                      which the call run lists its candidates (himut_call.h)
//   k_front_totals     the marked positions and column slots of a run over the column front, for the host's check of
//                      the kept capacities (the dbs and sites runs)
//
// Integer work (the proposals' trim limits are the only fp64); no MFMA.  Wave size 64 throughout.
#pragma once

#include "himut_emit.h"

namespace himut {

// ---------------------------------------------------------------------------------------
// propose_read: the proposals of one read.  Applies the read filters (caller.py:310-317) and, for every substitution that
// survives the trim and mismatch-window filters (bamlib.py:69-86,222-282) and every chunk that both contains tpos
// (caller.py:104-108,325) and fetched the read (caller.py:299), sets the (ref, alt) bit of the position in that
// chunk's mask -- the set() of caller.py:324.  The candidates are enumerated from the mask afterwards.  In a mask by
// chunk cell the proposal that sets a bit for the first time also counts it in its tile of 8192 mask cells: the scan of
// those counts is where k_mask_emit_cells puts each tile's candidates.
//
// It is the tail of k_stream_capture's wave: the wave that has streamed a read knows the read's quality sum, the last
// thing the read filters were waiting for, and what follows is a chain of dependent look-ups (chunk hint -> chunk
// records -> mismatch entries -> atomics) that costs a wave microseconds of latency and next to no bandwidth -- as a
// kernel of its own that chain, times the number of waves a chip holds, was 0.1 ms; behind a bandwidth-bound stream
// the other waves of the CU fill the time.
constexpr int EMIT_MAXC = 4;   // chunks of one read kept in registers
constexpr int PROP_TAB_BITS = 11;   // log2 of the entries of a recent-proposal table (propose_read's s_seen, where one is kept)

// The proposals of ONE read, by the sixteen lanes of a DPP row (gl = lane in the row, gsh = the row's first lane in
// the wave); the row takes the mismatch entries e0, e0 + estride, ...  (k_stream_capture calls it with the four rows of
// the read's wave: each row works out the read's chunks for itself, the rows share the entries.)  bqs: the sum of the
// read's qualities.  s_seen: the workgroup's recent-proposal table, or null.
__device__ __forceinline__ void propose_read(const Reads& R, const Derived& D, const Chunks& C, const Phase& H, const Params& P,
                                             const int64_t r, const uint32_t bqs, const int e0, const int estride, const int gl,
                                             const int gsh, uint32_t* mask, uint32_t* tilecnt, uint8_t* ccs_flag,
                                             unsigned long long* s_seen, const PosIndex& X, const int64_t rcells) {
    // the (ref, alt) bit of a mask cell: 16 mask bits per position, two positions per 32-bit word
    auto propose = [&](const int64_t cell, const int bit, const int64_t tile) {
        if (s_seen) {
            const unsigned long long key = ((unsigned long long)cell << 4) | (unsigned long long)bit;
            const uint32_t h = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - PROP_TAB_BITS));
            if (atomicExch(&s_seen[h], key) == key) return;
        }
        const uint32_t m = (1u << bit) << ((cell & 1) ? 16 : 0);
        if (tile < 0) atomicOr(mask + (cell >> 1), m);            // (nothing comes back: the wave does not wait for it)
        else if (!(atomicOr(mask + (cell >> 1), m) & m)) atomicAdd(tilecnt + tile, 1u);
    };
    // Where (chunk, tp1) has its cell.  By rank (rcells > 0, chunks in order): the position's column number + the chunk's
    // index; a cell past the rcells the mask holds is not written (the run's column slots then exceed the kept capacity,
    // and the run is made again); the bits are counted afterwards (k_mask_count).  Else by cell: the chunk's first cell +
    // the offset in the chunk, counted here in tiles of MASK_TILE_CELLS cells.
    const bool by_rank = rcells > 0;
    auto propose_at = [&](const int32_t chunk, const int64_t maskoff, const int32_t cstart, const int32_t tp1, const int bit,
                          const uint32_t u) {
        if (by_rank) {
            const int64_t cell = (int64_t)u + chunk;
            if (cell < rcells) propose(cell, bit, -1);
        } else {
            const int64_t cell = maskoff + (tp1 - cstart);
            propose(cell, bit, cell >> MASK_TILE_SHIFT);
        }
    };
    // cross-lane operations below stay inside the group: shuffles of width 16, the group's 16 bits of a ballot;
    // every branch around them is decided per read, i.e. uniform in the group
#define GBALLOT(P) ((uint32_t)((__ballot(P) >> gsh) & 0xffffull))
    const ReadMeta M = D.meta[r];
    const int32_t qlen = R.qlen[r];
    const int mapq = R.mapq[r];
    const int nm = D.nmis[r];
    const int32_t qid = R.qid[r];
    if (M.flags & RF_SECONDARY) return;
    const bool phase = P.p.phase != 0;
    bool live = (M.flags & RF_IDENT_OK) != 0;                             // bamlib.py:47-63, caller.py:314
    // np.mean(bq) < min_qv (bamlib.py:35, caller.py:310) in integers: for integers S, n, k the rounded quotient fl(S / n) is
    // below k exactly when S < k n (a quotient below k is below it by at least 1 / n, far more than half an ulp; rounding
    // is monotonic), and an empty query (0 / 0, not below anything) passes either way
    if (P.p.min_qv > 0 && (unsigned long long)bqs < (unsigned long long)P.p.min_qv * (unsigned long long)(uint32_t)qlen) live = false;
    if (mapq < P.p.min_mapq) live = false;
    if (!(P.p.qlen_lower_limit < qlen && qlen < P.p.qlen_upper_limit)) live = false;
    const int32_t ts = M.tstart, te = M.tend;

    // the chunks that fetched this read (start < tend and end > tstart): 15 records of the
    // sorted table around the look-up hint (and the one in front of them), one per lane, decided with one ballot
    int nc = 0;
    bool overflow = false;
    int64_t hi = 0;
    int32_t cc[EMIT_MAXC], cst[EMIT_MAXC], cen[EMIT_MAXC];
    int64_t cmo[EMIT_MAXC];
#pragma unroll
    for (int k = 0; k < EMIT_MAXC; k++) { cc[k] = -1; cst[k] = 0; cen[k] = -1; cmo[k] = 0; }
    if (live && C.n > 0) {
        const int64_t h0 = C.hint[min((int64_t)(te > 0 ? te : 0) >> CHUNK_HINT_SHIFT, C.nhint - 1)];
        const int64_t wlo = max(h0 - 8, (int64_t)0);
        const int64_t j = wlo - 1 + gl;                 // lane 0: the record in front of the window
        ChunkRec rec;
        rec.start = 0x7fffffff; rec.end = -0x7fffffff - 1; rec.idx = -1; rec.pmaxend = -0x7fffffff - 1; rec.maskoff = 0; rec.pairbase = 0;
        if (j >= 0 && j < C.n) rec = C.rec[j];
        // complete when no chunk in front of the window reaches the read and none behind it starts inside
        const bool front_ok = __shfl(rec.pmaxend, 0, 16) <= ts;
        const bool back_ok = wlo + 15 >= C.n || GBALLOT(gl >= 1 && rec.start >= te) != 0u;
        bool take = gl >= 1 && rec.idx >= 0 && rec.start < te && rec.end > ts;
        if (take && phase && H.hap[rec.pairbase + r] == HAP_NONE) take = false;     // caller.py:306-309
        const uint32_t tk = GBALLOT(take);
        nc = __popc(tk);
        if (!front_ok || !back_ok || nc > EMIT_MAXC) {
            // unusual chunk tables (deep nesting, a read across many chunks): walk the table per entry
            overflow = true;
            hi = h0;
            while (hi < C.n && C.rec[hi].start < te) hi++;
            nc = 0;
            for (int64_t jj = hi - 1; jj >= 0 && C.rec[jj].pmaxend > ts; jj--) {
                const ChunkRec q = C.rec[jj];
                if (q.end <= ts) continue;
                if (phase && H.hap[q.pairbase + r] == HAP_NONE) continue;
                nc++;
            }
        } else {
            uint32_t rest = tk;
#pragma unroll
            for (int k = 0; k < EMIT_MAXC; k++) {
                if (rest) {
                    const int src = __ffs((int)rest) - 1;
                    rest &= rest - 1;
                    cc[k] = __shfl(rec.idx, src, 16); cst[k] = __shfl(rec.start, src, 16); cen[k] = __shfl(rec.end, src, 16);
                    cmo[k] = ((int64_t)__shfl((int)(rec.maskoff >> 32), src, 16) << 32) | (uint32_t)__shfl((int)rec.maskoff, src, 16);
                }
            }
        }
        // num_ccs (caller.py:318-320): counted once it passes in any chunk that fetched it
        if (nc == 0) live = false;
        else if (gl == 0) ccs_flag[qid] = 1;
    } else live = false;

    if (!live) return;         // (the cs-vs-SEQ check of every substitution is k_parse_cs's)
    const int32_t* mis = D.mis + M.segbase;
    const uint32_t* mq = D.mq + M.segbase;
    const double trim_start = floor(P.p.min_trim * (double)qlen);        // bamlib.py:226
    const double trim_end = ceil((1.0 - P.p.min_trim) * (double)qlen);   // bamlib.py:227
    const int64_t w = P.p.mismatch_window_size;
    for (int e = e0; e < nm; e += estride) {
        const uint32_t v = mq[e];
        const int32_t tp1 = mis[e];
        const int32_t mprev = e > 0 ? mis[e - 1] : -0x7fffffff - 1;
        const int32_t mnext = e + 1 < nm ? mis[e + 1] : 0x7fffffff;
        if (!(v & 16u)) continue;                                             // substitutions only
        const int64_t q = v >> 5;
        if ((double)q < trim_start || (double)q > trim_end) continue;          // bamlib.py:231-242
        {                                                                     // bamlib.py:245-282
            int64_t qs = q - w, qe = q + w, ur, dr;
            if (qs < 0) { ur = w + qs; dr = w - qs; }
            else if (qe > qlen) { ur = w + (qe - qlen); dr = qlen - q; }
            else { ur = w; dr = w; }
            const int32_t ms = (int32_t)(tp1 - ur), me = (int32_t)(tp1 + dr);
            // bisect_right(me) - bisect_left(ms) - 1 on the sorted list; the entry itself is inside [ms, me]
            int lo = e, up = e + 1;
            if (mprev >= ms) { lo = e - 1; while (lo > 0 && mis[lo - 1] >= ms) lo--; }
            if (mnext <= me) { up = e + 2; while (up < nm && mis[up] <= me) up++; }
            if ((int64_t)(up - lo) - 1 > P.p.max_mismatch_count) continue;
        }
        const int bit = (int)(v & 15u);
        const uint32_t u = by_rank ? pos_rank(X, tp1 - 1) : 0u;               // (a proposal's position is marked: k_parse_cs)
        if (!overflow) {
#pragma unroll
            for (int k = 0; k < EMIT_MAXC; k++)
                if (cc[k] >= 0 && cst[k] <= tp1 && tp1 <= cen[k]) propose_at(cc[k], cmo[k], cst[k], tp1, bit, u);
        } else {
            for (int64_t jj = hi - 1; jj >= 0 && C.rec[jj].pmaxend > ts; jj--) {
                const ChunkRec qr = C.rec[jj];
                if (qr.end <= ts || !(qr.start <= tp1 && tp1 <= qr.end)) continue;
                if (phase && H.hap[qr.pairbase + r] == HAP_NONE) continue;
                propose_at(qr.idx, qr.maskoff, qr.start, tp1, bit, u);
            }
        }
    }
#undef GBALLOT
}

// Column positions and column-store slots per 256-position block, taken straight from the bitmap and the read
// windows (block_counts); their two prefix sums are each block's first rank and its slot offset.
struct BlockCount {
    const uint32_t* bits;
    const int32_t *winlo, *winhi;
};

// ---- the column index: the two prefix sums as two plain kernels.  k_block_sums leaves per-workgroup totals; in
// k_block_table3 every workgroup adds up the (at most 1024) totals in front of it, scans its own blocks and writes
// their block table.  A thread takes `per` consecutive blocks (1 unless the contig has more than 2^18 blocks).
__device__ __forceinline__ void block_counts(const BlockCount& F, int64_t b, uint32_t& cnt, uint32_t& nr, unsigned long long& slots) {
    const uint4* wp = reinterpret_cast<const uint4*>(F.bits + (b << 3));
    const uint4 x = wp[0], y = wp[1];
    cnt = (uint32_t)(__popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w) + __popc(y.x) + __popc(y.y) + __popc(y.z) + __popc(y.w));
    nr = (uint32_t)(F.winhi[b] - F.winlo[b]);
    slots = ((unsigned long long)cnt * (unsigned long long)nr + 15ULL) & ~15ULL;   // every block starts on a 32-byte boundary of the column store
}
// sums of (a, b) over the workgroup (256 threads), the same value in every thread
__device__ __forceinline__ void wg_sum2(uint32_t& a, unsigned long long& b, uint32_t* s_a, unsigned long long* s_b) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { a += __shfl_xor(a, d, 64); b += __shfl_xor(b, d, 64); }
    const int wv = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { s_a[wv] = a; s_b[wv] = b; }
    __syncthreads();
    a = s_a[0] + s_a[1] + s_a[2] + s_a[3];
    b = s_b[0] + s_b[1] + s_b[2] + s_b[3];
}
__global__ void __launch_bounds__(256) k_block_sums(BlockCount F, int64_t nblk, int per, uint4* part) {
    __shared__ uint32_t s_a[4];
    __shared__ unsigned long long s_b[4];
    const int64_t b0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * per;
    uint32_t c = 0;
    unsigned long long s = 0;
    for (int k = 0; k < per; k++)
        if (b0 + k < nblk) { uint32_t cnt, nr; unsigned long long sl; block_counts(F, b0 + k, cnt, nr, sl); c += cnt; s += sl; }
    wg_sum2(c, s, s_a, s_b);
    if (threadIdx.x == 0) part[blockIdx.x] = make_uint4(c, 0u, (uint32_t)s, (uint32_t)(s >> 32));
}
// BlockTab (first rank, slot offset) of every block; also leaves the slot offsets / counts as plain arrays (the run's
// totals).  err: HIMUT_ERR_DEPTH when the column store of the contig needs more than 2^32 slots or a window holds more
// than 2^22 reads.
__global__ void __launch_bounds__(256) k_block_table3(BlockCount F, int64_t nblk, int per, const uint4* part, BlockTab* bt,
                                                      uint32_t* blkoff, uint32_t* blkslots, int* err) {
    __shared__ uint32_t s_a[4];
    __shared__ unsigned long long s_b[4];
    // what the workgroups in front of this one hold
    uint32_t pc = 0;
    unsigned long long ps = 0;
    for (int w = threadIdx.x; w < (int)blockIdx.x; w += 256) {
        const uint4 v = part[w];
        pc += v.x; ps += (unsigned long long)v.z | ((unsigned long long)v.w << 32);
    }
    wg_sum2(pc, ps, s_a, s_b);
    // this thread's blocks, then the threads in front of it
    const int64_t b0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * per;
    uint32_t tc = 0;
    unsigned long long ts = 0;
    for (int k = 0; k < per; k++)
        if (b0 + k < nblk) { uint32_t cnt, nr; unsigned long long sl; block_counts(F, b0 + k, cnt, nr, sl); tc += cnt; ts += sl; }
    uint32_t ic = tc;
    unsigned long long is = ts;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t uc = __shfl_up(ic, d, 64);
        const unsigned long long us = __shfl_up(is, d, 64);
        if (lane >= d) { ic += uc; is += us; }
    }
    __syncthreads();
    if (lane == 63) { s_a[wv] = ic; s_b[wv] = is; }
    __syncthreads();
    uint32_t rc = pc + ic - tc;
    unsigned long long rs = ps + is - ts;
    for (int w = 0; w < wv; w++) { rc += s_a[w]; rs += s_b[w]; }
    bool deep = false;
    for (int k = 0; k < per; k++) {
        const int64_t b = b0 + k;
        if (b >= nblk) break;
        uint32_t cnt, nr;
        unsigned long long sl;
        block_counts(F, b, cnt, nr, sl);
        BlockTab t;
        t.lo = F.winlo[b]; t.ncnt = nr | (cnt << 22); t.boff = (uint32_t)rs; t.ufirst = rc;
        bt[b] = t;
        blkoff[b] = (uint32_t)rs; blkslots[b] = (uint32_t)sl;
        if (nr > BT_N_MASK || rs + sl > 0xffffffffULL) deep = true;
        rc += cnt; rs += sl;
    }
    if (deep) set_err(err, HIMUT_ERR_DEPTH);
}

// What the host of a run over the column front compares with the kept capacities, into two of the run's own scalars:
// the marked positions and the column-store slots of the run.
__global__ void k_front_totals(PosIndex X, const uint32_t* blkoff, const uint32_t* blkslots, unsigned long long* sc, int i_marked, int i_slots) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const FrontTotals t = front_totals_of(X, blkoff, blkslots);
    sc[i_marked] = t.marked; sc[i_slots] = t.slots;
}

struct CaptureArgs {
    Reads R;
    Derived D;
    PosIndex X;
    uint16_t* colstore;
    int64_t nslots;
    int64_t r_begin, r_end;      // reads of this launch
    uint32_t* bqsum;             // call path: per read, the sum of the qualities of the whole query (bamlib.py:34-36)
    const int* err;              // a device error raised by an earlier kernel of the run: nothing is captured then
    // call path: the read's proposals follow its stream (propose_read); mask null = none
    Chunks C;
    Phase H;
    Params P;
    uint32_t *mask, *tilecnt;
    uint8_t* ccs_flag;
    int64_t rcells;              // cells of a mask indexed by column rank (0: indexed by chunk cell), propose_read
};

constexpr int CLQ = 512;    // marked positions a wave keeps at a time: 16-bit offsets from the list's first word
constexpr int CSG = 63;     // segments per LDS window (+ 1 sentinel = one per lane)
constexpr int CWQ = 2048;   // query bases per window
constexpr int CPL = 256;    // reference positions per lane when the bitmap is enumerated (eight words): 64 lanes take 16 k
                            // positions per pass, a read's span in one or two
constexpr int CPD = 2;      // windows in flight (register sets); the loop is unrolled by it

// One wave per read; a software pipeline over windows of 2048 query bases.
//
// Window k is [c_k, c_k + 2048) of the query.  The segment list turns it into a reference
// range [tA_k, tB_k) (a deleted position goes with the base that follows it); those ranges
// tile the read's span.  The read's marked positions (the bitmap of column positions under its span) are listed once,
// 16 k positions a turn, as 16-bit offsets in LDS (refill).  Every turn of the loop
//   * stores the window's bytes -- 2 KB of qualities + 1 KB of packed bases, loaded two
//     turns earlier (CPD) with 16-byte coalesced loads -- in LDS,
//   * issues the same four loads for window k + CPD (three for the bytes, one for the block table under it): the
//     addresses depend only on the segment list, never on loaded data, so nothing in the loop waits on a
//     load younger than CPD turns and the count of loads in flight is the same every turn,
//   * takes the list's next entries below tB_k, one per lane: segment from a cursor that walks the list once, query
//     offset, base and quality out of the window in LDS, slot from the block table.
// Every byte of the read is fetched exactly once; stores return nothing.
#ifndef HIMUT_CAP_WAVES
#define HIMUT_CAP_WAVES 7
#endif
__device__ __forceinline__ void capture_wave(const CaptureArgs& A) {
    __shared__ __align__(16) uint8_t s_bq[4][CWQ];
    __shared__ __align__(16) uint8_t s_sq[4][CWQ / 2];
    __shared__ __align__(16) int4 s_seg[4][CSG + 1];
    __shared__ __align__(16) uint32_t s_bt[4][64];        // 16 block-table entries
    __shared__ uint16_t s_list[4][CLQ];
    const int tid = threadIdx.x, lane = tid & 63, wv = uni(tid >> 6);
    const Reads& R = A.R;
    const PosIndex& X = A.X;
    const int64_t r64 = A.r_begin + (int64_t)blockIdx.x * 4 + wv;
    if (r64 >= A.r_end || uni(*A.err)) return;
    const int32_t r = (int32_t)r64;
    const ReadMeta Mv = A.D.meta[r];
    const int32_t qlen = uni(R.qlen[r]);
    if (uni(Mv.flags) & RF_SECONDARY) return;
    if (uni(Mv.nseg) <= 0) {                 // nothing aligned (an empty cs tag): only the quality sum is wanted
        if (A.bqsum) {
            const uint8_t* q = R.bq + uni(Mv.qoff);
            uint32_t sum = 0;
            for (int32_t i = lane; i < qlen; i += 64) sum += q[i];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
            if (lane == 0) A.bqsum[r] = sum;
            if (A.mask) propose_read(R, A.D, A.C, A.H, A.P, r, uni(sum), lane, 64, lane & 15, lane & 48, A.mask, A.tilecnt, A.ccs_flag, nullptr, A.X, A.rcells);
        }
        return;
    }
    const Seg* gsegs = A.D.segs + uni(Mv.segbase);
    const int ns = uni(Mv.nseg);
    const int64_t qo = uni(Mv.qoff);
    const int32_t tstart = uni(Mv.tstart), tend = uni(Mv.tend);
    uint8_t* wbq = s_bq[wv];
    uint8_t* wsq = s_sq[wv];
    int4* lseg = s_seg[wv];
    uint32_t* lbt = s_bt[wv];
    uint16_t* list = s_list[wv];
    const bool all_lds = ns <= CSG;     // the whole segment list fits the LDS window

    // the windows start at query offset 0, soft clip included: the quality mean of the read filter is over the
    // whole query (a window in front of the aligned part has an empty reference range)
    const int nwin = ((max(qlen, 1) - 1) >> 11) + 1;
    uint32_t qsum = 0;     // this lane's share of the sum of the read's qualities
    const int32_t qpad = (qlen + 31) & ~31;

    // a load inside a rarely taken branch is waited for inside that branch, so that the join behind it
    // does not have to wait for every load in flight
#define CAP_LANDED4(V) asm volatile("" : "+v"(V.x), "+v"(V.y), "+v"(V.z), "+v"(V.w))
    // the four loads of one window (addresses clamped into the read, so every lane always loads)
#define CAP_ISSUE(BA, BB, SQ, BT, K, TA) do { \
        const int32_t _c = min((K), nwin - 1) * CWQ; \
        const int32_t _qa = min(_c + lane * 16, qpad - 16), _qb = min(_c + 1024 + lane * 16, qpad - 16), _qs = min(_c + lane * 32, qpad - 32); \
        BA = *reinterpret_cast<const uint4*>(R.bq + qo + _qa); \
        BB = *reinterpret_cast<const uint4*>(R.bq + qo + _qb); \
        SQ = *reinterpret_cast<const uint4*>(R.seq + ((qo + _qs) >> 1)); \
        BT = reinterpret_cast<const uint32_t*>(X.bt + min((int64_t)((TA) >> 8) + (lane >> 2), X.nblk - 1))[lane & 3]; \
    } while (0)
#define CAP_SEGWIN() do { if (lane <= nw) { int4 z = make_int4(0x7fffffff, 0, 0, 0); if (jb + lane < ns) z = *reinterpret_cast<const int4*>(gsegs + jb + lane); \
        lseg[lane] = z; } } while (0)

    // segment window [jb, jb + nw) plus a sentinel that carries the next segment's start
    int jb = 0, nw = min(ns, CSG);
    CAP_SEGWIN();
    uint4 ba0, bb0, sq0, ba1, bb1, sq1;
    uint32_t bt0r, bt1r;
    CAP_ISSUE(ba0, bb0, sq0, bt0r, 0, tstart);
    // rank of the first column position at or behind tstart: the block's first rank + the bits in front of tstart
    const uint32_t rk0 = uni(X.bt[min((int64_t)(tstart >> 8), X.nblk - 1)].ufirst) +
                         uni(pos_rank_in_block(X.bits, (int32_t)min((int64_t)tstart, (X.nblk << 8) - 1) & ~31));
    __builtin_amdgcn_wave_barrier();

    // end of window kk in reference coordinates: the first position whose query offset is >= c
    int jq = 0;   // no segment before jq ends behind the last boundary asked for
    auto window_end = [&](int kk) -> int32_t {
        if (kk >= nwin - 1) return tend + 1;
        const int32_t c = (kk + 1) * CWQ;
        while (true) {
            int4 sg = make_int4(tend + 1, 0x7ffffff0, 0, (int)SEG_DEL);        // behind the list: ends nowhere
            if (jq + lane < ns) {
                if (all_lds) sg = lseg[jq + lane];
                else { sg = *reinterpret_cast<const int4*>(gsegs + jq + lane); CAP_LANDED4(sg); }
            }
            const bool isrun = !((uint32_t)sg.w & SEG_DEL) && sg.z > 0;
            const int32_t qend = isrun ? sg.y + sg.z : sg.y + 1;
            const unsigned long long bal = __ballot(qend > c);
            if (bal) {
                const int src = __ffsll((long long)bal) - 1;
                const int32_t t0 = lane_val(sg.x, src), q0 = lane_val(sg.y, src);
                const bool inside = lane_val((int)(isrun && sg.y < c), src) != 0;
                jq += src;
                return inside ? t0 + (c - q0) : t0;
            }
            jq += 64;
        }
    };
    // ta[i] = first reference position of window k + i
    int32_t ta[CPD + 1];
    ta[0] = tstart;
    ta[1] = window_end(0);
    CAP_ISSUE(ba1, bb1, sq1, bt1r, 1, ta[1]);
    ta[2] = window_end(1);
    // ---- the read's marked positions, taken from the bitmap 16 k positions at a time (a read's span in one or two turns)
    //      into a list the windows then consume in order: list[i] = position - lbase, entries i_list .. n_list - 1 not yet
    //      used, all the marked positions of [.., covB) are in it or done with; u_list = the rank of list[0] among the
    //      contig's marked positions (the column's number: the block's first rank + what lies in front of tstart in it)
    int32_t covB = tstart, lbase = tstart & ~31;
    uint32_t u_list = rk0;
    int n_list = 0, i_list = 0;
    bool first_fill = true;
    auto refill = [&]() {
        u_list += (uint32_t)n_list; n_list = 0; i_list = 0;
        lbase = covB & ~31;
        for (int pass = 0; pass < 4 && covB <= tend; pass++) {          // (offsets stay below 2^16)
            const int32_t s0 = covB & ~31;
            const int64_t w0 = ((int64_t)s0 >> 5) + 8 * lane;
            uint32_t w[8];
            {
                uint4 a = make_uint4(0, 0, 0, 0), b = make_uint4(0, 0, 0, 0);
                if (w0 + 8 <= X.nwords + 2) {                               // (nwords + 2 words are allocated)
                    __builtin_memcpy(&a, X.bits + w0, 16);
                    __builtin_memcpy(&b, X.bits + w0 + 4, 16);
                } else {
                    uint32_t t[8];
#pragma unroll
                    for (int i = 0; i < 8; i++) t[i] = (w0 + i < X.nwords) ? X.bits[w0 + i] : 0u;
                    a = make_uint4(t[0], t[1], t[2], t[3]); b = make_uint4(t[4], t[5], t[6], t[7]);
                }
                w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
            }
            if (first_fill) {       // what the block's rank does not count yet: the bits of tstart's word in front of it
                u_list += (uint32_t)__popc((uint32_t)lane_val((int)w[0], 0) & ((1u << (tstart & 31)) - 1u));
                first_fill = false;
            }
            // positions in front of covB (they lie in the first word of lane 0) and behind tend (the read's last turn) are not
            // the read's
            const int32_t p_lane = s0 + CPL * lane;
            if (lane == 0) w[0] &= 0xffffffffu << (covB - s0);
            const int32_t keep = tend + 1 - p_lane;                        // this lane's leading positions that are the read's
            if (__ballot(keep < CPL)) {
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const int32_t ki = keep - 32 * i;
                    if (ki < 32) w[i] &= ki <= 0 ? 0u : ((1u << ki) - 1u);
                }
            }
            int cnt = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) cnt += __popc(w[i]);
            const int incl = wave_incl_add(cnt, lane);
            // the lanes whose positions still fit the list, from lane 0 on
            const unsigned long long fitb = __ballot(n_list + incl <= CLQ);
            const int L = fitb == ~0ULL ? 64 : (int)__builtin_ctzll(~fitb);
            if (lane < L) {
                int at = n_list + incl - cnt;
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    uint32_t b = w[i];
                    const int32_t off = p_lane + 32 * i - lbase;
                    while (b) { const int k = __ffs((int)b) - 1; b &= b - 1; list[at++] = (uint16_t)(off + k); }
                }
            }
            if (L > 0) n_list += lane_val(incl, L - 1);
            covB = s0 + CPL * L;
            if (L < 64) break;                                              // the list is full up to here
        }
        if (covB > tend) covB = tend + 1;
        __builtin_amdgcn_wave_barrier();
    };
    int jcur = 0;          // segment cursor of the candidate walk

    auto window = [&](uint4& ba, uint4& bb, uint4& sq, uint32_t& btv, const int k) {
        const int32_t tA = ta[0], tB = ta[1];
        const int32_t cq = k * CWQ;
        // ---- this window's bytes and tables -> LDS; its registers take window k + 2
        *reinterpret_cast<uint4*>(wbq + lane * 16) = ba;
        *reinterpret_cast<uint4*>(wbq + 1024 + lane * 16) = bb;
        *reinterpret_cast<uint4*>(wsq + lane * 16) = sq;
        lbt[lane] = btv;                                   // lane = entry * 4 + field
        {
            // np.mean(bq_int_lst) of caller.py:310 / bamlib.py:34-36: the bytes are here anyway.  A window behind the
            // read (k >= nwin) holds a reloaded copy of the last one; bytes behind qlen are masked off
            if (k < nwin) {
                if (cq + CWQ <= qlen) {
                    qsum = __builtin_amdgcn_sad_u8(ba.x, 0u, qsum); qsum = __builtin_amdgcn_sad_u8(ba.y, 0u, qsum);
                    qsum = __builtin_amdgcn_sad_u8(ba.z, 0u, qsum); qsum = __builtin_amdgcn_sad_u8(ba.w, 0u, qsum);
                    qsum = __builtin_amdgcn_sad_u8(bb.x, 0u, qsum); qsum = __builtin_amdgcn_sad_u8(bb.y, 0u, qsum);
                    qsum = __builtin_amdgcn_sad_u8(bb.z, 0u, qsum); qsum = __builtin_amdgcn_sad_u8(bb.w, 0u, qsum);
                } else {
                    const uint32_t wa[4] = {ba.x, ba.y, ba.z, ba.w}, wb_[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int ra = qlen - (cq + lane * 16 + 4 * i), rb = ra - 1024;   // bytes of the word inside the read
                        uint32_t xa = wa[i], xb = wb_[i];
                        if (ra < 4) xa = ra <= 0 ? 0u : (xa & (0xffffffffu >> (8 * (4 - ra))));
                        if (rb < 4) xb = rb <= 0 ? 0u : (xb & (0xffffffffu >> (8 * (4 - rb))));
                        qsum = __builtin_amdgcn_sad_u8(xa, 0u, qsum);
                        qsum = __builtin_amdgcn_sad_u8(xb, 0u, qsum);
                    }
                }
            }
        }
        CAP_ISSUE(ba, bb, sq, btv, k + CPD, ta[CPD]);
        const int32_t ta_next = window_end(k + CPD);
        __builtin_amdgcn_wave_barrier();
        const int64_t btb = tA >> 8;
        // one candidate per lane: segment, cell value, slot, store
        auto batch = [&](const bool act, const uint32_t rpos, const uint32_t u, const int32_t rlast) {
            // the segment that holds rpos = the last one that starts at or before it.  Candidates come
            // in reference order, so one cursor walks the list once per read (wave-uniform LDS reads)
            int4 sg = make_int4(0, 0, 0, 0);   // t0, q0, len, flags
            {
                int j = jcur;
                while (j < ns) {
                    if (j < jb || j >= jb + nw) {    // lists longer than the LDS window: reload it from j
                        jb = j; nw = min(ns - jb, CSG);
                        __builtin_amdgcn_wave_barrier();
                        CAP_SEGWIN();
                        __builtin_amdgcn_wave_barrier();
                    }
                    const int4 t = lseg[j - jb];
                    if (uni(t.x) > rlast) break;
                    if (act && (int32_t)rpos >= t.x) sg = t;
                    j++;
                }
                jcur = max(j - 1, jcur);
            }
            if (act) {
                const int32_t d = (int32_t)rpos - sg.x;
                const uint32_t insb = (d == 0 && ((uint32_t)sg.w & SEG_INS)) ? CELL_INS : 0u;
                bool store = false;
                uint32_t val = 0;
                if ((uint32_t)sg.w & SEG_DEL) { if (d < sg.z) { store = true; val = CELL_DEL | insb; } }
                else if (sg.z == 0) { if (d == 0 && insb) { store = true; val = CELL_EMPTY | CELL_INS; } }
                else if (d < sg.z) {
                    store = true;
                    const int32_t q = sg.y + d;
                    const int32_t o = (q - cq) & (CWQ - 1);       // inside the window by construction
                    const uint32_t qv = wbq[o], sb = wsq[o >> 1];
                    const int nib = (q & 1) ? (int)(sb & 15u) : (int)(sb >> 4);
                    val = insb | (uint32_t)nib2allele(nib) | (qv << 8);
                }
                if (store) {
                    const int64_t bi = (int64_t)(rpos >> 8) - btb;
                    uint4 t;
                    if (bi >= 0 && bi < 16) t = *reinterpret_cast<const uint4*>(lbt + 4 * bi);
                    else { t = *reinterpret_cast<const uint4*>(X.bt + min((int64_t)(rpos >> 8), X.nblk - 1)); CAP_LANDED4(t); }
                    // BlockTab: x = lo, y = n | cnt << 22, z = boff, w = ufirst
                    const int64_t slot = (int64_t)t.z + (int64_t)(r - (int32_t)t.x) * (int64_t)(t.y >> 22) + (int64_t)(u - t.w);
                    if ((uint64_t)slot < (uint64_t)A.nslots) A.colstore[slot] = (uint16_t)val;
                }
            }
        };
        // ---- the marked positions of [tA, tB): the next entries of the list, a lane each (a window holds about twenty);
        //      the list is filled again where the window reaches beyond what it covers
        while (true) {
            const int32_t hiP = min(tB, covB);
            int32_t e = 0x7fffffff;
            if (i_list + lane < n_list) e = lbase + (int32_t)list[i_list + lane];
            const bool act = e < hiP;
            const int bn = (int)__popcll(__ballot(act));                     // (the list is in order: the first bn lanes)
            if (bn) {
                batch(act, (uint32_t)e, u_list + (uint32_t)(i_list + lane), lane_val(e, bn - 1));
                i_list += bn;
            }
            if (bn == 64) continue;
            if (tB <= covB || covB > tend) break;
            __builtin_amdgcn_wave_barrier();
            refill();
        }
#pragma unroll
        for (int i = 0; i < CPD; i++) ta[i] = ta[i + 1];
        ta[CPD] = ta_next;
    };

    // CPD windows per trip, each with its own registers; the last ones of a trip may lie behind the
    // read (empty range): it still issues its loads, so the number in flight never depends on the path
    for (int k = 0; k < nwin; k += CPD) {
        window(ba0, bb0, sq0, bt0r, k);
        window(ba1, bb1, sq1, bt1r, k + 1);
    }
    if (A.bqsum) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) qsum += __shfl_down(qsum, d, 64);
        if (lane == 0) A.bqsum[r] = qsum;
        // a read with a base outside ATGC somewhere (k_flag_bases): KeyError in the reference if the base is aligned and
        // some chunk fetches the read (caller.py:57,299)
        if (R.nonacgt && uni((int)R.nonacgt[r])) {
            int64_t lo_ = 0, hi_ = A.C.n;
            while (lo_ < hi_) { const int64_t m_ = (lo_ + hi_) >> 1; if (A.C.rec[m_].start < tend) lo_ = m_ + 1; else hi_ = m_; }
            if (lo_ > 0 && A.C.rec[lo_ - 1].pmaxend > tstart && __ballot(!aligned_bases_ok(R, gsegs, ns, qo, lane, 64)))
                set_err(const_cast<int*>(A.err), HIMUT_ERR_BASE);
        }
        // the read filters have their last input: this read's proposals
        if (A.mask) propose_read(R, A.D, A.C, A.H, A.P, r, uni(qsum), lane, 64, lane & 15, lane & 48, A.mask, A.tilecnt, A.ccs_flag, nullptr, A.X, A.rcells);
    }
#undef CAP_ISSUE
#undef CAP_SEGWIN
#undef CAP_LANDED4
}

// (the wave's code as an inlined function of the argument block, not as the kernel's own body: as the body the compiler
// allocates registers differently and makes other code of it -- profiles/README.md, "Front split")
__global__ void __launch_bounds__(256, HIMUT_CAP_WAVES) k_stream_capture(CaptureArgs A) { capture_wave(A); }

}  // namespace himut
