// The kernels of himut_run_support (himut_support.hip): which reads carry each substitution of a site list, one row per
// (site, supporting read).  The contract is include/himut_hip.h (himut_run_support) and DESIGN.md section 8, row 7.
//
//   k_support<false>   count pass: per site the covering and the supporting reads
//   k_support_scan     the first row of every site (exclusive scan of the supporting reads), the total
//   k_support<true>    fill pass: the rows, within a site in the order the waves arrive
//   k_support_order    every row to its place: within a site ascending by read
#pragma once

#include "himut_device.h"

namespace himut {

static_assert(sizeof(himut_support_row) == 48, "himut_support_row is 48 bytes (SUPPORT_ROW_DTYPE of _ffi.py)");
static_assert(offsetof(himut_support_row, flag) == 24 && offsetof(himut_support_row, mapq) == 26 &&
              offsetof(himut_support_row, bq) == 27 && offsetof(himut_support_row, qpos) == 28 &&
              offsetof(himut_support_row, window_mismatches) == 44, "himut_support_row layout");

struct SupportArgs {
    Reads R;
    Derived D;
    const int32_t* pos1;      // the sites: 1-based position ascending
    const uint8_t* code;      // ref << 2 | alt in allele indices (A0 T1 G2 C3): the low four bits of a substitution's mq[] entry
    int64_t nsites;
    int32_t min_mapq, window;
    int32_t* counts;          // per site {cover, alt_reads}
    const int64_t* rowoff;    // fill pass: first row of every site
    uint32_t* cursor;         // fill pass: rows of the site written so far
    himut_support_row* rows;  // fill pass
};

// One wave per read, lanes over the sites the read covers (tstart <= pos1 - 1 < tend), 64 at a time.  A lane's site is
// supported when the read's mismatch list holds a substitution at pos1 with the site's (ref, alt): a binary search for
// the position, then the entries that share it (an insertion in front of a position is an entry at the same position).
// FILL: the rows.  What a row says about the whole read -- the quality sum, the substitution and indel counts -- is
// worked out by the wave together, once, and only by a wave that has a row to write.
template <bool FILL>
__global__ void __launch_bounds__(256) k_support(SupportArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + uni((int)(threadIdx.x >> 6));
    if (r >= A.R.n) return;
    const ReadMeta Mv = A.D.meta[r];
    const int mapq = uni((int)A.R.mapq[r]);
    if ((uni(Mv.flags) & RF_SECONDARY) || mapq < A.min_mapq) return;
    const int32_t tstart = uni(Mv.tstart), tend = uni(Mv.tend);
    const int64_t idx = uni(upper_bound(A.pos1, (int64_t)0, A.nsites, tstart)), jdx = uni(upper_bound(A.pos1, (int64_t)0, A.nsites, tend));
    const int64_t k = jdx - idx;
    if (k <= 0) return;
    const int nm = uni(A.D.nmis[r]);
    const int64_t sb = uni(Mv.segbase);
    const int32_t* mis = A.D.mis + sb;
    const uint32_t* mq = A.D.mq + sb;
    bool have_read = false;                // FILL: the whole-read figures below are known
    uint32_t bq_sum = 0;
    int n_sub = 0;
    for (int64_t a0 = 0; a0 < k; a0 += 64) {
        const int64_t g = idx + a0 + lane;
        const bool active = a0 + lane < k;
        bool hit = false;
        int32_t p = 0, qpos = 0;
        if (active) {
            p = A.pos1[g];
            const uint32_t want = 16u | (uint32_t)A.code[g];
            for (int e = (int)lower_bound(mis, (int64_t)0, (int64_t)nm, p); e < nm && mis[e] == p; e++) {
                const uint32_t v = mq[e];
                if ((v & 31u) == want) { hit = true; qpos = (int32_t)(v >> 5); }
            }
            if (!FILL) {
                atomicAdd(A.counts + 2 * g, 1);
                if (hit) atomicAdd(A.counts + 2 * g + 1, 1);
            }
        }
        if (!FILL) continue;
        if (!__ballot(hit)) continue;
        const int32_t qlen = uni(A.R.qlen[r]);
        const int64_t qo = uni(Mv.qoff);
        if (!have_read) {
            bq_sum = wave_bq_sum(A.R.bq + qo, qlen, lane);
            int ns = 0;
            for (int e = lane; e < nm; e += 64) ns += (mq[e] & 16u) ? 1 : 0;
            n_sub = lane_val(wave_incl_add(ns, lane), 63);
            have_read = true;
        }
        if (hit) {
            int64_t s, e;
            mismatch_range(p, qpos, qlen, A.window, s, e);
            himut_support_row row;
            row.site = (int32_t)g; row.read = (int32_t)r; row.qid = A.R.qid[r];
            row.tstart = tstart; row.tend = tend; row.qlen = qlen;
            row.flag = A.R.flag[r]; row.mapq = (uint8_t)mapq; row.bq = A.R.bq[qo + qpos];
            row.qpos = qpos; row.bq_sum = bq_sum; row.n_sub = n_sub; row.n_indel = nm - n_sub;
            row.window_mismatches = mismatches_in(mis, nm, s, e) - 1;
            const int64_t slot = A.rowoff[g] + (int64_t)atomicAdd(A.cursor + g, 1u);
            if (slot < A.rowoff[g + 1]) A.rows[slot] = row;      // (the count pass saw the same reads: always)
        }
    }
}

// One workgroup: rowoff[g] = supporting reads of the sites in front of g, rowoff[nsites] = *total = all of them.  A
// thread sums a run of consecutive sites, the workgroup scans the 256 sums, the thread writes its run.
__global__ void __launch_bounds__(256) k_support_scan(const int32_t* counts, int64_t nsites, int64_t* rowoff, unsigned long long* total) {
    __shared__ int64_t s_sum[256];
    const int tid = threadIdx.x;
    const int64_t per = (nsites + 255) / 256;
    const int64_t g0 = min(nsites, tid * per), g1 = min(nsites, g0 + per);
    int64_t sum = 0;
    for (int64_t g = g0; g < g1; g++) sum += counts[2 * g + 1];
    s_sum[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int64_t acc = 0;
        for (int t = 0; t < 256; t++) { const int64_t v = s_sum[t]; s_sum[t] = acc; acc += v; }
        rowoff[nsites] = acc;
        *total = (unsigned long long)acc;
    }
    __syncthreads();
    int64_t acc = s_sum[tid];
    for (int64_t g = g0; g < g1; g++) { rowoff[g] = acc; acc += counts[2 * g + 1]; }
}

// A thread per row: its place within its site = the site's rows with a smaller read (a read has one row per site).
__global__ void __launch_bounds__(256) k_support_order(const himut_support_row* in, const int64_t* rowoff, int64_t nsites, int64_t nrows, himut_support_row* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrows) return;
    const uint4* src = reinterpret_cast<const uint4*>(in + i);       // a row is three 16-byte pieces: site and read lead the first
    const uint4 r0 = src[0], r1 = src[1], r2 = src[2];
    const int32_t site = (int32_t)r0.x, read = (int32_t)r0.y;
    if (site < 0 || site >= nsites) return;                          // (never: the fill pass wrote every row)
    const int64_t b = rowoff[site], e = rowoff[site + 1];
    int64_t rank = 0;
    for (int64_t j = b; j < e; j++) rank += in[j].read < read ? 1 : 0;
    uint4* dst = reinterpret_cast<uint4*>(out + b + rank);
    dst[0] = r0; dst[1] = r1; dst[2] = r2;
}

}  // namespace himut
