// libhimut_hip.so: signature exposures with bootstrap replicates (himut_fit_exposures) over the kernels of himut_fit.h.
// The call reads nothing of the context but its stream, events and scratch pools: no reads, reference, site sets or
// parameters, and it changes none of them.
#include <hip/hip_runtime.h>

#include <cmath>

#include "himut_ctx.h"
#include "himut_fit.h"

using namespace himut;

namespace {

constexpr unsigned FIT_MAX_WGS = 2048;          // the grid's cap: the kernels stride over more replicates (himut_debug_fit)

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

inline unsigned fit_grid(const himut_ctx* c, int64_t n) {
    const unsigned cap = c->dbg_fit_wgs > 0 ? (unsigned)c->dbg_fit_wgs : FIT_MAX_WGS;
    return (unsigned)std::min<int64_t>(std::max<int64_t>(n, 1), cap);
}

}  // namespace

extern "C" {

int himut_fit_exposures(himut_ctx* c, const double* sig, int32_t C, int32_t K, const int64_t* counts, int32_t n_boot,
                        uint64_t seed, int32_t iters, double* exposures, int32_t* resampled) {
    if (!c) return HIMUT_ERR_ARG;
    if (!sig || !counts || !exposures) return fail(c, HIMUT_ERR_ARG, "himut_fit_exposures: a null array");
    if (C < 1 || C > FIT_MAX_C) return fail(c, HIMUT_ERR_ARG, "himut_fit_exposures: C outside 1..1536");
    if (K < 1 || K > FIT_MAX_K) return fail(c, HIMUT_ERR_ARG, "himut_fit_exposures: K outside 1..96");
    if (n_boot < 0 || n_boot > FIT_MAX_BOOT) return fail(c, HIMUT_ERR_ARG, "himut_fit_exposures: n_boot outside 0..100000");
    if (iters < 1 || iters > FIT_MAX_ITERS) return fail(c, HIMUT_ERR_ARG, "himut_fit_exposures: iters outside 1..100000");
    return guarded(c, [&]() -> int {
        std::vector<int32_t> m((size_t)C);
        std::vector<uint32_t> prefix((size_t)C);
        int64_t N = 0;
        for (int32_t i = 0; i < C; i++) {
            if (counts[i] < 0) return fail(c, HIMUT_ERR_ARG, "himut_fit_exposures: count " + std::to_string(i) + " is negative");
            if (counts[i] > INT32_MAX || (N += counts[i]) > INT32_MAX)
                return fail(c, HIMUT_ERR_ARG, "himut_fit_exposures: the counts sum to 2^31 or more");
            m[i] = (int32_t)counts[i];
            prefix[i] = (uint32_t)N;
        }
        for (size_t i = 0; i < (size_t)C * K; i++)
            if (!std::isfinite(sig[i]) || sig[i] < 0.0)
                return fail(c, HIMUT_ERR_ARG, "himut_fit_exposures: sig[" + std::to_string(i / K) + "][" + std::to_string(i % K) +
                                                  "] is negative or not finite");
        HCHECK(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        const size_t n_rep = (size_t)n_boot + 1;
        // d_tmp: the matrix, the counts, their prefix sums; d_tmp2: the replicates' counts, the exposures
        const size_t o_m = align256((size_t)C * K * 8), o_pre = o_m + align256((size_t)C * 4);
        const size_t o_expo = align256(n_rep * C * 4);
        c->d_tmp.reserve(o_pre + (size_t)C * 4 + 256);
        c->d_tmp2.reserve(o_expo + n_rep * K * 8 + 256);
        double* d_sig = c->d_tmp.as<double>();
        int32_t* d_m = reinterpret_cast<int32_t*>(c->d_tmp.as<uint8_t>() + o_m);
        uint32_t* d_pre = reinterpret_cast<uint32_t*>(c->d_tmp.as<uint8_t>() + o_pre);
        int32_t* d_rep = c->d_tmp2.as<int32_t>();
        double* d_expo = reinterpret_cast<double*>(c->d_tmp2.as<uint8_t>() + o_expo);
        // the workgroup of k_fit_em: S in LDS with as many replicates (waves) beside it as the budget holds, if it holds one;
        // else S from global memory and as many replicates as the budget holds, at least one
        const size_t budget = c->dbg_fit_lds > 0 ? (size_t)c->dbg_fit_lds : (size_t)FIT_LDS_BUDGET;
        const size_t per_rep = fit_rep_bytes(C, K);
        const size_t sig_lds = (size_t)C * fit_row_stride(K) * 8;
        const bool s_in_lds = sig_lds + per_rep <= budget;
        const int waves = (int)std::min<size_t>(std::max<size_t>((budget - (s_in_lds ? sig_lds : 0)) / per_rep, 1), FIT_WAVES);
        const size_t em_lds = waves * per_rep + (s_in_lds ? sig_lds : 0);
        HCHECK(hipEventRecord(c->ev[EV_SIDE], st));
        HCHECK(hipMemcpyAsync(d_sig, sig, (size_t)C * K * 8, hipMemcpyHostToDevice, st));
        HCHECK(hipMemcpyAsync(d_m, m.data(), (size_t)C * 4, hipMemcpyHostToDevice, st));
        HCHECK(hipMemcpyAsync(d_pre, prefix.data(), (size_t)C * 4, hipMemcpyHostToDevice, st));
        HCHECK(hipEventRecord(c->ev[EV_START], st));
        hipLaunchKernelGGL(k_fit_resample, dim3(fit_grid(c, (int64_t)n_rep)), dim3(256), (size_t)C * 8, st, d_m, d_pre, (int)C,
                           (uint32_t)N, (int)n_boot, seed, d_rep);
        HCHECK(hipGetLastError());
        HCHECK(hipEventRecord(c->ev[EV_HAP], st));
        const dim3 em_grid(fit_grid(c, (int64_t)((n_rep + waves - 1) / waves))), em_block(64 * waves);
        const double e0 = (double)N / (double)K;
        if (s_in_lds)
            hipLaunchKernelGGL(k_fit_em<true>, em_grid, em_block, em_lds, st, d_sig, (int)C, (int)K, d_rep, (int)n_rep, e0, (int)iters, d_expo);
        else
            hipLaunchKernelGGL(k_fit_em<false>, em_grid, em_block, em_lds, st, d_sig, (int)C, (int)K, d_rep, (int)n_rep, e0, (int)iters, d_expo);
        HCHECK(hipGetLastError());
        HCHECK(hipEventRecord(c->ev[EV_FINAL], st));
        HCHECK(hipMemcpyAsync(exposures, d_expo, n_rep * K * 8, hipMemcpyDeviceToHost, st));
        if (resampled) HCHECK(hipMemcpyAsync(resampled, d_rep, n_rep * C * 4, hipMemcpyDeviceToHost, st));
        HCHECK(hipStreamSynchronize(st));
        memset(&c->stats, 0, sizeof(c->stats));
        c->stats.ms_total = elapsed_ms(c, EV_START, EV_FINAL);      // himut_get_stats: the two kernels,
        c->stats.ms_hap = elapsed_ms(c, EV_START, EV_HAP);          // k_fit_resample,
        c->stats.ms_eval = elapsed_ms(c, EV_HAP, EV_FINAL);         // k_fit_em,
        c->stats.ms_parse = elapsed_ms(c, EV_SIDE, EV_START);       // the upload in front of them
        c->stats.n_candidates = (int64_t)n_rep;
        c->stats.n_unique_positions = em_grid.x;                    // workgroups of k_fit_em,
        c->stats.n_records = waves;                                 // replicates that share a workgroup of k_fit_em,
        c->stats.column_slots = (int64_t)em_lds;                    // its LDS bytes,
        c->stats.positions = s_in_lds ? (int64_t)sig_lds : 0;       // those of them that hold S (0: S is read from global memory)
        return HIMUT_OK;
    });
}

int himut_debug_fit(himut_ctx* c, int max_workgroups, int lds_budget_bytes) {
    if (!c) return HIMUT_ERR_ARG;
    if (max_workgroups < 0 || lds_budget_bytes < 0 || lds_budget_bytes > FIT_LDS_BUDGET)
        return fail(c, HIMUT_ERR_ARG, "himut_debug_fit: max_workgroups below 0 or lds_budget_bytes outside 0..65536");
    c->dbg_fit_wgs = max_workgroups;
    c->dbg_fit_lds = lds_budget_bytes;
    return HIMUT_OK;
}

}  // extern "C"
