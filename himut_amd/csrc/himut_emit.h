// The record back end that the runs over the column front share: where a record goes (wg_rank), how a himut_record is
// packed (pack_record), how the records are moved to the front (k_compact_runs, the one compaction kernel of the germline
// and dbs runs) and what a run leaves for the host's check of the kept capacities (front_totals_of).  A run's records
// come out in thread order within a workgroup and workgroup order across: a kernel that gives thread t of workgroup w
// item w * NT + t of an ordered list emits its records in that order.
#pragma once

#include "himut_column.h"

namespace himut {

struct WgRank { int rank, total; };      // the items of the threads in front of this one; of the whole workgroup

// behind the barrier that follows the waves' totals in s_w: in_wave + the waves in front of this thread's, and all of them
template <int NW>
__device__ __forceinline__ WgRank wg_rank_sum(const int in_wave, const int* s_w) {
    WgRank r{in_wave, 0};
#pragma unroll
    for (int k = 0; k < NW; k++) { if (k < (int)(threadIdx.x >> 6)) r.rank += s_w[k]; r.total += s_w[k]; }
    return r;
}

// The rank of an emitting thread among the emitting threads of its workgroup of NW waves, in thread order, and their
// number.  s_w: one word per wave.  One workgroup barrier, for every thread, between the waves' totals and their sums; a
// caller that uses s_w again (a next round) puts a barrier in between.
template <int NW>
__device__ __forceinline__ WgRank wg_rank(const bool emit, int* s_w) {
    const int lane = threadIdx.x & 63;
    const unsigned long long b = __ballot(emit);
    if (lane == 0) s_w[threadIdx.x >> 6] = (int)__popcll(b);
    __syncthreads();
    return wg_rank_sum<NW>((int)__popcll(b & ((1ULL << lane) - 1ULL)), s_w);
}

// the same for a thread with n items (the germline run's position list: the set bits of a bitmap word)
template <int NW>
__device__ __forceinline__ WgRank wg_rank_count(const int n, int* s_w) {
    const int lane = threadIdx.x & 63, incl = wave_incl_add(n, lane);
    if (lane == 63) s_w[threadIdx.x >> 6] = incl;
    __syncthreads();
    return wg_rank_sum<NW>(incl - n, s_w);
}

// ---- himut_record as four 16-byte stores; the alleles are 0..3 (ATGC order) and are written as letters
static_assert(sizeof(himut_record) == 64 && offsetof(himut_record, tpos) == 0 && offsetof(himut_record, chunk) == 4 &&
              offsetof(himut_record, phase_set) == 8 && offsetof(himut_record, gq) == 12 && offsetof(himut_record, ref) == 16 &&
              offsetof(himut_record, alt) == 17 && offsetof(himut_record, gt0) == 18 && offsetof(himut_record, gt1) == 19 &&
              offsetof(himut_record, status) == 20 && offsetof(himut_record, gt_state) == 21 && offsetof(himut_record, flags) == 22 &&
              offsetof(himut_record, counts) == 24 && offsetof(himut_record, bqsum) == 48, "pack_record places every field of himut_record");
// the flags byte inside the second 32-bit word of word 1 (status, gt_state, flags, pad): k_compact clears it
constexpr uint32_t REC_W1Y_FLAGS_SHIFT = 8 * (offsetof(himut_record, flags) - offsetof(himut_record, status));
constexpr uint32_t REC_W1Y_FLAGS_MASK = 0xffu << REC_W1Y_FLAGS_SHIFT;

struct RecordWords {
    uint4 w[4];
    __device__ __forceinline__ void store(himut_record* dst) const {
        uint4* d = reinterpret_cast<uint4*>(dst);
        d[0] = w[0]; d[1] = w[1]; d[2] = w[2]; d[3] = w[3];
    }
};

__device__ __forceinline__ RecordWords pack_record(const int32_t tpos, const int32_t chunk, const int32_t phase_set, const int32_t gq,
                                                   const int ref, const int alt, const int g0, const int g1, const int status,
                                                   const int gt_state, const uint32_t flags, const uint32_t* cnt, const uint32_t* bqs) {
    RecordWords r;
    r.w[0] = make_uint4((uint32_t)tpos, (uint32_t)chunk, (uint32_t)phase_set, (uint32_t)gq);
    r.w[1] = make_uint4((uint32_t)allele2char(ref) | ((uint32_t)allele2char(alt) << 8) | ((uint32_t)allele2char(g0) << 16) |
                            ((uint32_t)allele2char(g1) << 24),
                        (uint32_t)(status & 255) | ((uint32_t)gt_state << 8) | (flags << REC_W1Y_FLAGS_SHIFT), cnt[0], cnt[1]);
    r.w[2] = make_uint4(cnt[2], cnt[3], cnt[4], cnt[5]);
    r.w[3] = make_uint4(bqs[0], bqs[1], bqs[2], bqs[3]);
    return r;
}

// ---- what the host of a run over the column front compares with the kept capacities: the marked positions (the last
// block's first rank + its marked positions) and the column-store slots (the end of the last block) of the run
struct FrontTotals { unsigned long long marked, slots; };
__device__ __forceinline__ FrontTotals front_totals_of(const PosIndex& X, const uint32_t* blkoff, const uint32_t* blkslots) {
    const BlockTab t = X.bt[X.nblk - 1];
    return {(unsigned long long)t.ufirst + (unsigned long long)(t.ncnt >> 22),
            (unsigned long long)blkoff[X.nblk - 1] + (unsigned long long)blkslots[X.nblk - 1]};
}

// ---- Workgroup w of an eval kernel left wgcnt[w] records in thread order somewhere of its own; this moves them behind
// the records of the workgroups in front of it (every workgroup adds up the counts in front of it), and the last one
// leaves the record count.  One workgroup of 256 threads per workgroup of the eval kernel.  First::src(w, mine):
// workgroup w's first record; may lower `mine` (w's count, not 0) to what can be there, or return null: nothing is
// moved.  First::tail(): what else the launch leaves, for every thread.
template <class Rec, class First>
__global__ void __launch_bounds__(256) k_compact_runs(const uint32_t* wgcnt, const First first, Rec* out, unsigned long long* nrec) {
    static_assert(sizeof(Rec) % 16 == 0, "records are moved in 16-byte words");
    __shared__ unsigned long long s_sum[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned long long part = 0;
    for (int64_t k = tid; k < (int64_t)blockIdx.x; k += 256) part += wgcnt[k];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d, 64);
    if (lane == 0) s_sum[wv] = part;
    __syncthreads();
    const unsigned long long base = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    uint32_t mine = wgcnt[blockIdx.x];
    const Rec* from = mine ? first.src((int64_t)blockIdx.x, mine) : nullptr;
    if (from) {
        const uint4* src = reinterpret_cast<const uint4*>(from);
        uint4* dst = reinterpret_cast<uint4*>(out + base);
        for (int64_t k = tid; k < (int64_t)mine * (int64_t)(sizeof(Rec) / 16); k += 256) dst[k] = src[k];
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) *nrec = base + mine;
    first.tail();
}

// The First of a run whose eval kernel gives every workgroup 256 slots of its own (dbs, indels): workgroup w's records
// start at slot w * 256, no more than 256 of them, and the launch leaves nothing else.
template <class Rec>
struct SlotRuns {
    const Rec* recs;
    __device__ __forceinline__ const Rec* src(int64_t w, uint32_t& mine) const { mine = min(mine, 256u); return recs + w * 256; }
    __device__ __forceinline__ void tail() const {}
};

}  // namespace himut
