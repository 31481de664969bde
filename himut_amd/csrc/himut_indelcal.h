// Device code of the indelcal run (himut_run_indelcal): per homopolymer run of the reference, the pile reads that span it
// and the indel events the reads show in it.  The contract is include/himut_hip.h (himut_run_indelcal) and DESIGN.md
// section 8, row 13.
//
// The run starts from the indels run's ordered events (k_indel_events, the sort, k_indel_order: himut_indels.h) and adds
// three kernels over them and over the reference string:
//
//   k_indelcal_mark    one thread per ordered event, the first of an allele works: n_alt and DP as k_indel_eval counts
//                      them (allele_tally); an allele at or above the thresholds sets its anchor's bit in a position bitmap
//   k_indelcal_events  one thread per ordered event: variant anchor, off run, partial, or its class and column
//                      (allele_class, the function k_indel_eval reads a table with); the 128 x 7 histogram in LDS, one
//                      global atomic per cell that counted and workgroup
//   k_indelcal_spans   the dense half: a workgroup at a time per 256 anchor positions.  The letters of the block and of the 80
//                      positions behind it go to LDS as codes; one thread per anchor finds whether a run starts behind it
//                      and how long it is; the block's window reads (winlo / winhi: every read that can span an anchor
//                      of the block) go through LDS 256 at a time, as (tstart, tend) of the pile reads, and every thread
//                      with a run counts the ones that span it -- any number of reads, any read length; the 128 x 3
//                      histogram (runs, excluded, spans) stays in LDS over all the blocks of a workgroup (a resident
//                      grid strides over the blocks): one global atomic per cell that counted and workgroup
//   k_indelcal_blocks  in front of it, per block: does a region hold one, or all, of its anchors
#pragma once

#define HIMUT_INDELS_NO_KERNELS
#include "himut_indels.h"

namespace himut {

static_assert(sizeof(himut_indelcal_params) == 32, "himut_indelcal_params is 32 bytes (IndelcalParams of _ffi.py)");
static_assert(RUN_CLASSES == HIMUT_INDELCAL_CLASSES && RUN_CELLS == HIMUT_INDEL_ERROR_CELLS, "the table's shape is the header's");

constexpr int IC_COLS = HIMUT_INDELCAL_COLS;     // runs excluded spans del1 del2 del3p ins1 ins2 ins3p other
constexpr int IC_COL_RUNS = 0, IC_COL_EXCLUDED = 1, IC_COL_SPANS = 2, IC_COL_EVENTS = 3;
constexpr int IC_TABLE = RUN_CLASSES * IC_COLS;
// the run's own words behind the IND_SC_WORDS of the event front: the table, then the counters the kernels keep
constexpr int IC_W_TABLE = 0, IC_W_CNT = IC_TABLE;
constexpr int IC_CNT_ANCHORS = 0, IC_CNT_VARIANT_ANCHORS = 1, IC_CNT_EV_VARIANT = 2, IC_CNT_OFFRUN = 3, IC_CNT_PARTIAL = 4,
              IC_CNT_RUNS_LONG = 5, IC_NCNT = 8;
constexpr int IC_WORDS = IC_TABLE + IC_NCNT;
constexpr int IC_STAGE = 256;                    // window reads k_indelcal_spans holds in LDS at a time
constexpr int IC_REF = 256 + 80;                 // letters it holds: an anchor's run ends at most RUN_MAX + 2 behind it

struct IndelcalArgs {
    IndelArgs A;                                 // the ordered events, the reads, the reference string, the regions, the windows
    int32_t min_alt_count, vaf_permille;
    int64_t nblk;                                // blocks winlo / winhi hold
    uint64_t cell_budget;                        // k_indelcal_spans flushes its LDS histogram before a cell could pass this (2^31)
    int64_t blk0, nb;                            // k_indelcal_spans: the first block of the sweep, their number
    uint32_t* bits;                              // bit a: anchor a is variant
    uint8_t* blkflag;                            // k_indelcal_blocks: per block of the sweep, from blk0
    unsigned long long* w;                       // IC_WORDS words
};

__device__ __forceinline__ bool is_variant(const uint32_t* bits, int32_t a) { return (bits[a >> 5] >> (a & 31)) & 1u; }

__global__ void __launch_bounds__(256) k_indelcal_mark(IndelcalArgs C) {
    const IndelArgs& A = C.A;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= A.nev || *A.err) return;
    const IndelEvent E = A.ord[j];
    const int32_t a = (int32_t)(E.key >> IND_KEY_SHIFT);
    bool first_of_allele = true;
    if (j > 0) {
        const IndelEvent B = A.ord[j - 1];
        first_of_allele = !same_allele(B, E);
        if ((int32_t)(B.key >> IND_KEY_SHIFT) != a) atomicAdd(C.w + IC_W_CNT + IC_CNT_ANCHORS, 1ull);
    } else {
        atomicAdd(C.w + IC_W_CNT + IC_CNT_ANCHORS, 1ull);
    }
    if (!first_of_allele) return;
    const AlleleTally T = allele_tally(A, j, E);
    if ((int64_t)T.n_alt >= C.min_alt_count && (int64_t)T.n_alt * 1000 >= (int64_t)C.vaf_permille * T.dp) {
        const uint32_t bit = 1u << (a & 31);
        if (!(atomicOr(C.bits + (a >> 5), bit) & bit)) atomicAdd(C.w + IC_W_CNT + IC_CNT_VARIANT_ANCHORS, 1ull);
    }
}

__global__ void __launch_bounds__(256) k_indelcal_events(IndelcalArgs C) {
    __shared__ uint32_t s_hist[RUN_CELLS];
    __shared__ uint32_t s_cnt[IC_NCNT];
    const IndelArgs& A = C.A;
    const int tid = threadIdx.x;
    for (int i = tid; i < RUN_CELLS; i += 256) s_hist[i] = 0;
    if (tid < IC_NCNT) s_cnt[tid] = 0;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + tid;
    if (j < A.nev && !*A.err) {
        const IndelEvent E = A.ord[j];
        const int32_t a = (int32_t)(E.key >> IND_KEY_SHIFT);
        if (is_variant(C.bits, a)) {
            atomicAdd(&s_cnt[IC_CNT_EV_VARIANT], 1u);
        } else {
            int n = 0;
            const int cell = allele_class(A.refseq, A.reflen, a, (int)((E.key >> 6) & 1u), (int)(E.key & 63u) + 1, E.s0, E.s1, &n);
            if (cell < 0) atomicAdd(&s_cnt[IC_CNT_OFFRUN], 1u);
            else if (!(a + 1 + n < A.D.meta[E.read].tend)) atomicAdd(&s_cnt[IC_CNT_PARTIAL], 1u);
            else atomicAdd(&s_hist[cell], 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i < RUN_CELLS; i += 256)
        if (s_hist[i]) atomicAdd(C.w + IC_W_TABLE + (i / RUN_EVCOLS) * IC_COLS + IC_COL_EVENTS + i % RUN_EVCOLS, (unsigned long long)s_hist[i]);
    if (tid < IC_NCNT && s_cnt[tid]) atomicAdd(C.w + IC_W_CNT + tid, (unsigned long long)s_cnt[tid]);
}

// Per 256-position block of the sweep: 0 no region holds one of its anchors, 1 some region does, 2 one region holds them
// all (no thread of the block has to look its anchor up).  A kernel of its own, so that the look-ups of all blocks run side
// by side: in front of each workgroup of the sweep, two binary searches of dependent loads were most of the sweep's time.
__global__ void __launch_bounds__(256) k_indelcal_blocks(IndelcalArgs C, int64_t nb) {
    const IndelArgs& A = C.A;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nb) return;
    const int64_t p0 = (C.blk0 + i) << WIN_SHIFT;
    const int32_t last = (int32_t)(p0 + 255);
    const int64_t k = upper_bound(A.s_start, (int64_t)0, A.nregion, last);
    uint8_t live = k > 0 && (int64_t)A.s_pmaxend[k - 1] >= p0;
    if (live) {
        const int64_t k0 = upper_bound(A.s_start, (int64_t)0, A.nregion, (int32_t)p0);
        if (k0 > 0 && A.s_pmaxend[k0 - 1] >= last) live = 2;
    }
    C.blkflag[i] = live;
}

__global__ void __launch_bounds__(256) k_indelcal_spans(IndelcalArgs C) {
    __shared__ uint32_t s_hist[RUN_CLASSES * 3];
    __shared__ int2 s_rd[IC_STAGE];
    __shared__ int8_t s_ref[IC_REF];
    __shared__ uint32_t s_long;
    const IndelArgs& A = C.A;
    const int tid = threadIdx.x, lane = tid & 63;
    if (*A.err) return;
    if (tid == 0) s_long = 0;
    for (int i = tid; i < RUN_CLASSES * 3; i += 256) s_hist[i] = 0;
    // the workgroup's counts to the table: one global atomic per cell that counted.  Every workgroup adds to the same few
    // words, and adds to one word take their turns: a workgroup per block did so 250,000 times per hot cell on the bench
    // workload, which was the whole of the sweep's 4.6 ms; a resident grid that keeps its histogram over its blocks does not.
    auto flush = [&]() {
        __syncthreads();
        for (int i = tid; i < RUN_CLASSES * 3; i += 256)
            if (s_hist[i]) {
                atomicAdd(C.w + IC_W_TABLE + (i / 3) * IC_COLS + i % 3, (unsigned long long)s_hist[i]);
                s_hist[i] = 0;
            }
        __syncthreads();
    };
    uint64_t budget = 0;                         // what a 32-bit cell can hold at most of the blocks since the last flush
    for (int64_t bi = blockIdx.x; bi < C.nb; bi += gridDim.x) {
        const int live = C.blkflag[bi];          // (the same word in every lane: no look-up in front of the block's loads)
        if (!live) continue;
        const bool all_in = live == 2;
        const int64_t blk = C.blk0 + bi;
        const int64_t p0 = blk << WIN_SHIFT;
        const int32_t rlo = blk < C.nblk ? A.winlo[blk] : 0, rhi = blk < C.nblk ? A.winhi[blk] : 0;
        budget += 256ull * (uint64_t)(rhi - rlo) + 256ull;
        if (budget > C.cell_budget) { flush(); budget = 256ull * (uint64_t)(rhi - rlo) + 256ull; }
        __syncthreads();                         // the previous block's letters have been read
        for (int i = tid; i < IC_REF; i += 256) {
            const int64_t p = p0 + i;
            s_ref[i] = (int8_t)(p < A.reflen ? char2allele(upper((int)A.refseq[p])) : -1);
        }
        __syncthreads();
        // ---- the run behind this thread's anchor
        const int64_t a = p0 + tid, s = a + 1;
        int b = 0;
        int n = run_at([&](int64_t i) { return (int)s_ref[i - p0]; }, A.reflen, s, &b);
        bool counting = false;
        int cls = 0;
        if (n > 0) {
            int64_t end = s + n;                 // a long run: where it ends is in the string alone
            if (n > RUN_MAX)
                while (end < A.reflen && char2allele(upper((int)A.refseq[end])) == b) end++;
            if (!(end < A.reflen) || !(all_in || in_region(A.s_start, A.s_pmaxend, A.nregion, (int32_t)a))) n = 0;
        }
        const bool has = n > 0 && n <= RUN_MAX;  // a run with a class
        if (has) {
            cls = run_class(b, n);
            counting = !is_variant(C.bits, (int32_t)a);
        }
        // ---- the pile reads that span it: the window's reads through LDS, IC_STAGE at a time
        const int32_t a32 = (int32_t)a, e32 = (int32_t)(s + n);
        uint32_t spans = 0;
        for (int32_t base = rlo; base < rhi; base += IC_STAGE) {
            __syncthreads();
            const int32_t r = base + tid;
            if (r < rhi) {
                const ReadMeta M = A.D.meta[r];
                const bool pile = !(M.flags & RF_SECONDARY) && !((int)A.R.mapq[r] < A.p.min_mapq);
                s_rd[tid] = pile ? make_int2(M.tstart, M.tend) : make_int2(INT32_MAX, INT32_MIN);
            }
            __syncthreads();
            const int m = min(IC_STAGE, rhi - base);
            if (counting)
                for (int k = 0; k < m; k++) {
                    const int2 v = s_rd[k];
                    spans += (uint32_t)(v.x <= a32 && e32 < v.y);
                }
        }
        // ---- the wave's runs class by class (an iid string puts most of a wave into a dozen classes): one LDS atomic per
        // class, column and wave, not three per thread on the same few cells
        const unsigned long long longs = __ballot(n > RUN_MAX);
        if (lane == 0 && longs) atomicAdd(&s_long, (uint32_t)__popcll(longs));
        unsigned long long todo = __ballot(has);
        while (todo) {
            const int lead = __ffsll((long long)todo) - 1;
            const int c = __shfl(cls, lead);
            const bool mine = has && cls == c;
            const unsigned long long same = __ballot(mine), excl = __ballot(mine && !counting);
            uint32_t sp = mine ? spans : 0u;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) sp += __shfl_xor(sp, d);
            if (lane == lead) {
                atomicAdd(&s_hist[c * 3 + IC_COL_RUNS], (uint32_t)__popcll(same));
                if (excl) atomicAdd(&s_hist[c * 3 + IC_COL_EXCLUDED], (uint32_t)__popcll(excl));
                if (sp) atomicAdd(&s_hist[c * 3 + IC_COL_SPANS], sp);
            }
            todo &= ~same;
        }
    }
    flush();
    if (tid == 0 && s_long) atomicAdd(C.w + IC_W_CNT + IC_CNT_RUNS_LONG, (unsigned long long)s_long);
}

}  // namespace himut
