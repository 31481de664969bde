// Device code of the sindels run (himut_run_sindels): somatic indel candidates carried by single reads.  The contract is
// include/himut_hip.h (himut_run_sindels) and DESIGN.md section 8, row 16.
//
// The run starts from the indels run's front (indel_front_run, himut_indels.hip) with three things of its own:
//
//   k_sindel_reads  between the decode and the events, a wave per pile read: the read's qualities once, sixteen bytes a
//                   lane and load, summed four bytes at a time (v_sad_u8; k_callable's pass A is the precedent), a wave
//                   reduction, and call's read filters as one byte per read (SR_PILE | SR_PROPOSES).  The front has no
//                   capture, which is where the other runs get the quality sums from.  A read that is not in the pile
//                   costs its metadata and no stream
//   k_indel_events<SomRules>  (himut_indels.h) the indels run's event kernel with the per-event rules -- trim, mismatch
//                   window, qualities of the footprint -- applied where the raw position and query offset are known; an
//                   event that passes carries EV_PROPOSES through the sort and k_indel_order
//   k_sindel_eval   one thread per ordered event, the first of an allele works: n_alt, n_other and DP (allele_tally),
//                   n_prop from its run of events, the run behind the anchor and the allele's class (run_at,
//                   allele_class), the three-state genotype in fp64 (indel_genotype, k_indel_eval's), the verdict
//                   cascade; the record goes out through wg_rank and k_compact_runs (himut_emit.h)
#pragma once

#define HIMUT_INDELS_NO_KERNELS
#include "himut_indels.h"

namespace himut {

static_assert(sizeof(himut_sindel_params) == 120, "himut_sindel_params is 120 bytes (SindelParams of _ffi.py)");
static_assert(offsetof(himut_sindel_params, l_hit) == 32 && offsetof(himut_sindel_params, qlen_lower_limit) == 80 &&
              offsetof(himut_sindel_params, min_sequence_identity) == 104, "himut_sindel_params layout");
static_assert(sizeof(himut_sindel_record) == 64, "himut_sindel_record is 64 bytes (SINDEL_RECORD_DTYPE of _ffi.py)");
static_assert(offsetof(himut_sindel_record, type) == offsetof(himut_indel_record, type) && offsetof(himut_sindel_record, gq) == offsetof(himut_indel_record, gq) &&
              offsetof(himut_sindel_record, dp) == offsetof(himut_indel_record, dp) && offsetof(himut_sindel_record, bases) == offsetof(himut_indel_record, bases) &&
              offsetof(himut_sindel_record, n_prop) == offsetof(himut_indel_record, reserved) && offsetof(himut_sindel_record, run_base) == 52,
              "himut_sindel_record keeps himut_indel_record's offsets");

// the run's own words behind the IND_SC_WORDS of the event front
constexpr int SIN_W_PILE = 0, SIN_W_PROPOSING = 1;   // k_sindel_reads
constexpr int SIN_W_EVAL = 2;                        // k_sindel_eval: candidates, germ het, germ hom-alt, then the six verdicts
constexpr int SIN_EV_CAND = 0, SIN_EV_GERM_HET = 1, SIN_EV_GERM_HOMALT = 2, SIN_EV_INDELSITE = 3, SIN_EV_REPEAT = 4, SIN_EV_LOWGQ = 5,
              SIN_EV_LOWDEPTH = 6, SIN_EV_HIGHDEPTH = 7, SIN_EV_PASS = 8, SIN_NEV = 9;
constexpr int SIN_WORDS = 16;
constexpr int SIN_NLOG = 20;                         // himut_get_sindels' counters

struct SindelReadArgs {
    Reads R;
    const ReadMeta* meta;
    int32_t min_mapq, min_qv, qlen_lower_limit, qlen_upper_limit;
    uint8_t* verdict;
    unsigned long long* w;       // SIN_WORDS words
    const int* err;
};

// The sum of the bytes [lo, hi) of bq, for the 64 lanes of a wave together (lo, hi wave-uniform): every lane's share.  The
// loads are the 16-byte pieces of the aligned span around [lo, hi), four of a lane in flight; the bytes of the first and
// the last piece that lie outside are masked.
__device__ __forceinline__ uint32_t wave_bq_share(const uint8_t* bq, const int64_t lo, const int64_t hi, const int lane) {
    uint32_t sum = 0;
    const int64_t a0 = lo & ~(int64_t)15;
    auto masked = [&](const uint4 v, const int64_t a) {    // the piece at a with the bytes outside [lo, hi) cleared
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t b = a + 4 * k;
            const int drop = (int)min(max(lo - b, (int64_t)0), (int64_t)4), keep = (int)min(max(hi - b, (int64_t)0), (int64_t)4);
            uint32_t m = keep >= 4 ? 0xffffffffu : (keep <= 0 ? 0u : (0xffffffffu >> (8 * (4 - keep))));
            m &= drop >= 4 ? 0u : (0xffffffffu << (8 * drop));
            w[k] &= m;
        }
        return make_uint4(w[0], w[1], w[2], w[3]);
    };
    for (int64_t a = a0 + (int64_t)lane * 16; a < hi; a += 4096) {
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t ak = a + 1024 * k;
            v[k] = ak < hi ? *reinterpret_cast<const uint4*>(bq + ak) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t ak = a + 1024 * k;
            if (ak < lo || ak + 16 > hi) v[k] = ak < hi ? masked(v[k], ak) : v[k];
            sum = __builtin_amdgcn_sad_u8(v[k].x, 0u, sum);
            sum = __builtin_amdgcn_sad_u8(v[k].y, 0u, sum);
            sum = __builtin_amdgcn_sad_u8(v[k].z, 0u, sum);
            sum = __builtin_amdgcn_sad_u8(v[k].w, 0u, sum);
        }
    }
    return sum;
}

__global__ void __launch_bounds__(256) k_sindel_reads(SindelReadArgs A) {
    __shared__ uint32_t s_cnt[2];
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + uni((int)(threadIdx.x >> 6));
    if (r < A.R.n && !*A.err) {
        const uint32_t flags = uni(A.meta[r].flags);
        const int mapq = uni((int)A.R.mapq[r]);
        uint8_t verdict = 0;
        if (!(flags & RF_SECONDARY) && !(mapq < A.min_mapq)) {
            verdict = SR_PILE;
            const int64_t qo = uni(A.R.qoff[r]);
            const int32_t qlen = uni(A.R.qlen[r]);
            uint64_t sum = wave_bq_share(A.R.bq, qo, qo + max(qlen, 0), lane);
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
            // call's read filters (caller.py:310-317), as propose_read and k_dbs_propose apply them
            const bool ok = (flags & RF_IDENT_OK) && !(sum < (uint64_t)(int64_t)max(A.min_qv, 0) * (uint64_t)(uint32_t)max(qlen, 0)) &&
                            A.qlen_lower_limit < qlen && qlen < A.qlen_upper_limit;
            if (ok) verdict |= SR_PROPOSES;
            if (lane == 0) {
                atomicAdd(&s_cnt[0], 1u);
                if (ok) atomicAdd(&s_cnt[1], 1u);
            }
        }
        if (lane == 0) A.verdict[r] = verdict;
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(A.w + SIN_W_PILE + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

struct SindelEvalArgs {
    IndelArgs A;                 // the ordered events and what allele_tally reads; A.p: the genotype's block
    int32_t max_run;
    himut_sindel_record* recs;   // workgroup w's records start at w * 256
    unsigned long long* w;       // SIN_WORDS words
};

__global__ void __launch_bounds__(256) k_sindel_eval(SindelEvalArgs C) {
    __shared__ uint32_t s_cnt[16];
    __shared__ int s_e[4];
    const IndelArgs& A = C.A;
    const int tid = threadIdx.x;
    if (tid < 16) s_cnt[tid] = 0;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + tid;
    bool emit = false;
    uint4 w0 = make_uint4(0, 0, 0, 0), w1 = w0, w2 = w0, w3 = w0;
    if (j < A.nev && !*A.err) {
        const IndelEvent E = A.ord[j];
        if (j == 0 || !same_allele(A.ord[j - 1], E)) {           // the first of its allele
            const AlleleTally T = allele_tally(A, j, E);
            // the distinct reads with a proposing event: reads ascending, a read's repeats are neighbours
            uint32_t n_prop = 0, prev = 0;
            bool prev_counted = false;
            for (uint32_t k = 0; k < T.run; k++) {
                const IndelEvent B = A.ord[j + k];
                if (k == 0 || B.read != prev) prev_counted = false;
                if ((B.first & EV_PROPOSES) && !prev_counted) { n_prop++; prev_counted = true; }
                prev = B.read;
            }
            if (n_prop > 0) {
                const uint32_t n_alt = T.n_alt, n_other = T.n_other, dp = T.dp;
                const int32_t a = (int32_t)(E.key >> IND_KEY_SHIFT);
                const int type = (int)((E.key >> 6) & 1u), L = (int)(E.key & 63u) + 1;
                const uint32_t n_non = dp - n_alt;
                int n_run = 0, run_b = 0;
                const int cell = allele_class(A.refseq, A.reflen, a, type, L, E.s0, E.s1, &n_run);
                if (n_run > 0) run_at([&](int64_t i) { return char2allele(upper((int)A.refseq[i])); }, A.reflen, (int64_t)a + 1, &run_b);
                const int col = cell >= 0 ? cell % RUN_EVCOLS : 255;
                double l_hit = A.p.l_hit, l_err = A.p.l_err;
                if (A.tab_hit && cell >= 0) { l_hit = A.tab_hit[cell]; l_err = A.tab_err[cell]; }
                const IndelGenotype G = indel_genotype(A.p, n_non, n_alt, l_hit, l_err);
                const int state = G.state, gq = G.gq;
                atomicAdd(&s_cnt[SIN_EV_CAND], 1u);
                if (state != 0) {
                    atomicAdd(&s_cnt[state == 1 ? SIN_EV_GERM_HET : SIN_EV_GERM_HOMALT], 1u);
                } else {
                    int status = HIMUT_ST_PASS, slot = SIN_EV_PASS;
                    if (n_other > 0) { status = HIMUT_ST_INDEL; slot = SIN_EV_INDELSITE; }
                    else if (n_run > RUN_MAX || (col < RUN_EVCOLS - 1 && n_run > C.max_run)) { status = HIMUT_ST_REPEAT; slot = SIN_EV_REPEAT; }
                    else if (gq < A.p.min_gq) { status = HIMUT_ST_LOWGQ; slot = SIN_EV_LOWGQ; }
                    else if ((int64_t)n_alt < A.p.min_alt_count || (int64_t)dp - n_alt - n_other < (int64_t)A.p.min_ref_count) { status = HIMUT_ST_LOWDEPTH; slot = SIN_EV_LOWDEPTH; }
                    else if ((int64_t)dp > A.p.md_threshold) { status = HIMUT_ST_HIGHDEPTH; slot = SIN_EV_HIGHDEPTH; }
                    atomicAdd(&s_cnt[slot], 1u);
                    emit = true;
                    w0 = make_uint4((uint32_t)a, (uint32_t)L, (uint32_t)type | ((uint32_t)status << 8), (uint32_t)gq);
                    w1 = make_uint4(dp, n_alt, n_other, 0u);
                    w2 = record_bases(E);
                    w3 = make_uint4(n_prop, (uint32_t)(n_run > 0 ? run_b : 0) | ((uint32_t)n_run << 8) | ((uint32_t)col << 16), 0u, 0u);
                }
            }
        }
    }
    // ---- the workgroup's records in thread (= allele) order
    const WgRank e = wg_rank<4>(emit, s_e);
    if (emit) {
        uint4* dst = reinterpret_cast<uint4*>(C.recs + ((int64_t)blockIdx.x * 256 + e.rank));
        dst[0] = w0; dst[1] = w1; dst[2] = w2; dst[3] = w3;
    }
    if (tid == 0) A.wgcnt[blockIdx.x] = (uint32_t)e.total;
    __syncthreads();
    if (tid < SIN_NEV && s_cnt[tid]) atomicAdd(C.w + SIN_W_EVAL + tid, (unsigned long long)s_cnt[tid]);
}

}  // namespace himut
