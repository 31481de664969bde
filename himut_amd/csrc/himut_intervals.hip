// libhimut_hip.so: the intervals run (himut_run_intervals, himut_get_intervals) over the kernels of himut_intervals.h.
// It reads what the last completed callable run left -- the map, its offsets, and the copies of that run's chunk list and
// reference length (himut_ctx::Callmap) -- and the context's reference string; the intervals, the plan and the rows are its
// own, so every other getter keeps serving its last run.  Nothing of it waits for the host before the last kernel.
#include <hip/hip_runtime.h>
#include <string.h>  // rocprim's texture iterator needs the host memset declared first
#include <rocprim/rocprim.hpp>

#include "himut_ctx.h"
#include "himut_intervals.h"

using namespace himut;

namespace {

int do_intervals(himut_ctx* c, const int32_t* start, const int32_t* end, int64_t n) {
    himut_ctx::Callmap& M = c->callmap;
    himut_ctx::Intervals& I = c->intervals;
    if (!M.have || !M.last_ok) return fail(c, HIMUT_ERR_ARG, "himut_run_intervals: no completed himut_run_callable to read the map of");
    if (n < 0) return fail(c, HIMUT_ERR_ARG, "himut_run_intervals: n < 0");
    if (n > 0 && (!start || !end)) return fail(c, HIMUT_ERR_ARG, "himut_run_intervals: start or end is null");
    if (c->reflen != M.g_reflen) return fail(c, HIMUT_ERR_ARG, "himut_run_intervals: the reference string is not as long as the one the callable run saw");
    begin_run(c, I.out);
    I.have = false;
    hipStream_t st = c->stream;
    const int64_t nch = (int64_t)M.g_cs.size();
    bool ordered = true;
    for (int64_t k = 0; k < nch && ordered; k++)
        ordered = M.g_cs[(size_t)k] <= M.g_ce[(size_t)k] && (k + 1 == nch || M.g_ce[(size_t)k] <= M.g_cs[(size_t)k + 1]);

    // ---- every buffer before anything is queued (DevBuf::reserve drains the device when it grows)
    const size_t words = ((size_t)n + 1) * sizeof(int64_t);
    I.d_lo.reserve(words); I.d_hi.reserve(words); I.d_chunks.reserve(words); I.d_cnt.reserve(words); I.d_off.reserve(words);
    I.d_rows.reserve((size_t)std::max<int64_t>(n, 1) * sizeof(himut_interval_row));
    long long* cnt = I.d_cnt.as<long long>();
    long long* off = I.d_off.as<long long>();
    auto scan = [&](void* tmp, size_t& bytes) {
        return rocprim::exclusive_scan(tmp, bytes, cnt, off, 0LL, (size_t)n + 1, rocprim::plus<long long>(), st);
    };
    sort_with_tmp(I.d_scantmp, false, scan);
    upload(I.d_start, start, (size_t)n, st);
    upload(I.d_end, end, (size_t)n, st);
    upload(I.d_cs, M.g_cs, st);
    upload(I.d_ce, M.g_ce, st);

    HCHECK(hipEventRecord(c->ev[EV_START], st));
    if (n > 0) {
        IvGeo G;
        G.cs = I.d_cs.as<int32_t>(); G.ce = I.d_ce.as<int32_t>(); G.mapoff = M.d_mapoff.as<int64_t>(); G.nch = nch;
        G.ordered = ordered ? 1 : 0;
        G.mstate = M.d_state.as<uint8_t>(); G.mbases = M.d_bases.as<uint16_t>();
        G.refseq = c->d_refseq.as<uint8_t>(); G.reflen = c->reflen;
        HCHECK(hipMemsetAsync(I.d_rows.p, 0, (size_t)n * sizeof(himut_interval_row), st));
        hipLaunchKernelGGL(k_iv_plan, dim3(blocks_for(n + 1, 256)), dim3(256), 0, st, G, I.d_start.as<int32_t>(), I.d_end.as<int32_t>(), n,
                           I.d_lo.as<int64_t>(), I.d_hi.as<int64_t>(), I.d_chunks.as<int2>(), cnt);
        sort_with_tmp(I.d_scantmp, true, scan);
        hipLaunchKernelGGL(k_iv_tally, dim3((unsigned)std::max(c->n_cus, 1) * 8u), dim3(IV_NT), 0, st, G, I.d_start.as<int32_t>(),
                           I.d_end.as<int32_t>(), n, I.d_lo.as<int64_t>(), I.d_hi.as<int64_t>(), I.d_chunks.as<int2>(), off,
                           I.d_rows.as<unsigned long long>());
    }
    HCHECK(hipEventRecord(c->ev[EV_FINAL], st));
    HCHECK(hipStreamSynchronize(st));
    HCHECK(hipGetLastError());
    I.out.n = n; I.have = true;
    himut_run_stats& S = c->stats;
    S.ms_total = elapsed_ms(c, EV_START, EV_FINAL);
    S.positions = M.n_pos; S.n_records = n;
    return HIMUT_OK;
}

}  // namespace

extern "C" {

int himut_run_intervals(himut_ctx* c, const int32_t* start, const int32_t* end, int64_t n) {
    if (!c) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int { return do_intervals(c, start, end, n); });
}

int himut_get_intervals(himut_ctx* c, const himut_interval_row** rows, int64_t* n) {
    if (!c || !rows || !n) return HIMUT_ERR_ARG;
    if (!c->intervals.have) return fail(c, HIMUT_ERR_ARG, "himut_run_intervals has not completed");
    return guarded(c, [&]() -> int { return get_run_out(c, c->intervals.out, c->intervals.d_rows, rows, n, (int64_t*)nullptr); });
}

}  // extern "C"
