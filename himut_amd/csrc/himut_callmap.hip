// libhimut_hip.so: the callable run (himut_run_callable, himut_get_callable, himut_get_callable_map) over the kernels of
// himut_callmap.h.  Its front is the normcounts run's, step for step (norm_plan as a whole-contig tile pass,
// norm_read_pass, norm_args: himut_norm.hip); the map, the runs and the scan's scratch are its own, and what
// himut_get_normcounts serves is left alone.  A completed run keeps a host copy of its chunk list and reference length:
// the intervals run (himut_intervals.hip) reads the map by them.
#include <hip/hip_runtime.h>

#include "himut_ctx.h"
#include "himut_callmap.h"

using namespace himut;

namespace {

int do_callable(himut_ctx* c, const uint8_t* alt_order, int non_human) {
    if (int rc = check_scan_inputs(c, true)) return rc;
    if (c->cstart.empty()) return fail(c, HIMUT_ERR_ARG, "himut_set_chunks has not been called: without chunks there is no map");
    for (int k = 0; k < 12; k++) if (alt_order[k] > 3) return fail(c, HIMUT_ERR_ARG, "alt_order holds alleles 0..3");
    if (c->cstart.size() > 65535) return fail(c, HIMUT_ERR_ARG, "more than 65,535 chunks in one contig (the sweep's grids take a chunk per row)");
    himut_ctx::Callmap& M = c->callmap;
    begin_run(c, M.out);
    M.have = false; M.n_pos = 0;
    c->params.unique_qnames = c->unique_qnames ? 1 : 0;
    hipStream_t st = c->stream;

    // ---- the plan: the front's buffers, then the map (the chunks' positions one behind the other) and the scan's blocks
    const NormPlan P = norm_plan(c, upload_chunks(c, c->cstart, c->cend), NormPass::Tile);
    const int64_t nch = (int64_t)c->cstart.size();
    std::vector<int64_t> mapoff((size_t)nch + 1, 0);
    for (int64_t k = 0; k < nch; k++) mapoff[(size_t)k + 1] = mapoff[(size_t)k] + ((int64_t)c->cend[(size_t)k] - c->cstart[(size_t)k]);
    const int64_t N = mapoff[(size_t)nch];
    const int64_t nblocks = (N + CM_BLOCK - 1) / CM_BLOCK;
    M.d_state.reserve((size_t)N + CM_BLOCK + 64);                      // (slack: the scan's threads load eight entries at a time)
    M.d_bases.reserve(((size_t)N + CM_BLOCK + 64) * 2);
    M.d_blk.reserve((size_t)(nblocks + 1) * sizeof(CmPair));
    M.d_sc.reserve(sizeof(CmScalars));
    upload(M.d_mapoff, mapoff, st);
    uint8_t* mstate = M.d_state.as<uint8_t>();
    uint16_t* mbases = M.d_bases.as<uint16_t>();
    const int64_t* d_mapoff = M.d_mapoff.as<int64_t>();
    CmScalars* cs = M.d_sc.as<CmScalars>();

    // ---- EV_START .. EV_EMIT: the read pass; .. EV_SWEEP: the map
    norm_read_pass(c, P);
    HCHECK(hipMemsetAsync(cs, 0, sizeof(CmScalars), st));
    if (P.work) {
        launch_count_flags(c, P.sc);
        const NormArgs A = norm_args(c, P, alt_order, non_human);
        const int64_t per = ((int64_t)blocks_for(P.maxspan, 256) + 7) / 8;
        const dim3 grid(8u * (unsigned)std::min<int64_t>(NT_Q, per), (unsigned)P.T.n);
        hipLaunchKernelGGL(k_callmap_sweep, grid, dim3(256), 0, st, A, P.D, c->norm.d_callable.as<uint32_t>(), c->d_winlo.as<int32_t>(),
                           c->d_winhi.as<int32_t>(), P.nblk, per, d_mapoff, mstate, mbases, &cs->deep);
    } else if (N > 0) {                                                 // no reads: the reference letter decides
        hipLaunchKernelGGL(k_callmap_noreads, dim3(blocks_for(N, 256)), dim3(256), 0, st, c->d_refseq.as<uint8_t>(), c->reflen,
                           c->d_cstart.as<int32_t>(), d_mapoff, nch, N, mstate, mbases, &P.sc->err);
    }
    stage_event(c, EV_SWEEP, 1, st);

    // ---- .. EV_GATHER: the runs.  The count first; the records are sized for exactly that many.
    if (N > 0) {
        hipLaunchKernelGGL(k_cm_reduce, dim3((unsigned)nblocks), dim3(CM_NT), 0, st, mstate, mbases, d_mapoff, nch, N, M.d_blk.as<CmPair>());
        hipLaunchKernelGGL(k_cm_scan, dim3(1), dim3(CM_SCAN_NT), 0, st, M.d_blk.as<CmPair>(), nblocks, cs);
    }
    CmScalars hc;
    Scalars hs;
    unsigned long long hlog[16];
    HCHECK(hipMemcpyAsync(&hc, cs, sizeof(CmScalars), hipMemcpyDeviceToHost, st));
    HCHECK(hipMemcpyAsync(&hs, P.sc, sizeof(Scalars), hipMemcpyDeviceToHost, st));
    HCHECK(hipMemcpyAsync(hlog, c->norm.d_tri.as<unsigned long long>() + 2 * P.ntri, sizeof(hlog), hipMemcpyDeviceToHost, st));
    HCHECK(hipStreamSynchronize(st));
    // (the read pass wrote the normcounts run's read-pass buffers: what himut_debug_norm_callable copies is this pass's now)
    if (c->norm.have) { c->norm.cal_words = P.work ? (c->bq_bytes >> 5) : 0; c->norm.cal_reads = P.work ? c->n : 0; }
    if (hs.err) return check_device_err(c, hs.err);
    if (hc.deep) return fail(c, HIMUT_ERR_DEPTH, "a position holds more than 65,535 callable bases: the map's bases field is 16 bits");
    const int64_t nruns = hc.nruns;
    M.d_bnd.reserve((size_t)(nruns + 1) * sizeof(CmPair));
    M.d_runs.reserve((size_t)std::max<int64_t>(nruns, 1) * sizeof(himut_callable_run));
    M.out.h.resize((size_t)nruns);
    if (N > 0) {
        hipLaunchKernelGGL(k_cm_bounds, dim3((unsigned)nblocks), dim3(CM_NT), 0, st, mstate, mbases, d_mapoff, nch, N, M.d_blk.as<CmPair>(), cs,
                           M.d_bnd.as<CmPair>());
        hipLaunchKernelGGL(k_cm_records, dim3(blocks_for(nruns, 256)), dim3(256), 0, st, mstate, d_mapoff, c->d_cstart.as<int32_t>(), nch,
                           M.d_bnd.as<CmPair>(), nruns, M.d_runs.as<himut_callable_run>());
    }
    stage_event(c, EV_GATHER, 1, st);
    if (nruns > 0)
        HCHECK(hipMemcpyAsync(M.out.h.data(), M.d_runs.p, (size_t)nruns * sizeof(himut_callable_run), hipMemcpyDeviceToHost, st));
    HCHECK(hipEventRecord(c->ev[EV_FINAL], st));
    HCHECK(hipStreamSynchronize(st));

    take_log(M.out, hlog);
    M.out.log[0] = (int64_t)hs.nccs;
    M.out.n = nruns; M.out.valid = true; M.n_pos = N; M.have = true;
    M.g_cs = c->cstart; M.g_ce = c->cend; M.g_reflen = c->reflen;         // (host only: what the intervals run reads the map by)
    himut_run_stats& S = c->stats;
    S.ms_total = elapsed_ms(c, EV_START, EV_FINAL);
    S.ms_index = elapsed_ms(c, EV_START, EV_EMIT);
    if (c->timing >= 1) {
        S.ms_eval = elapsed_ms(c, EV_EMIT, EV_SWEEP);
        S.ms_capture = elapsed_ms(c, EV_SWEEP, EV_GATHER);
        S.ms_finalize = elapsed_ms(c, EV_GATHER, EV_FINAL);
    }
    S.n_reads = c->n; S.read_bases = c->read_bases; S.positions = N; S.n_records = nruns;
    return HIMUT_OK;
}

}  // namespace

extern "C" {

int himut_run_callable(himut_ctx* c, const uint8_t* alt_order, int non_human_sample) {
    if (!c || !alt_order) return HIMUT_ERR_ARG;
    c->callmap.last_ok = false;
    const int rc = guarded(c, [&]() -> int { return do_callable(c, alt_order, non_human_sample); });
    c->callmap.last_ok = rc == HIMUT_OK;
    return rc;
}

int himut_get_callable(himut_ctx* c, const himut_callable_run** runs, int64_t* n_runs, int64_t log[14]) {
    if (!c || !runs || !n_runs) return HIMUT_ERR_ARG;
    if (!c->callmap.have) return fail(c, HIMUT_ERR_ARG, "himut_run_callable has not completed");
    return guarded(c, [&]() -> int { return get_run_out(c, c->callmap.out, c->callmap.d_runs, runs, n_runs, log); });
}

int himut_get_callable_map(himut_ctx* c, uint8_t* state, uint16_t* bases, int64_t n) {
    if (!c) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int {
        const himut_ctx::Callmap& M = c->callmap;
        if (!M.have) return fail(c, HIMUT_ERR_ARG, "himut_run_callable has not completed");
        if (n < 0 || n > M.n_pos) return fail(c, HIMUT_ERR_ARG, "himut_get_callable_map: more entries than the run swept");
        HCHECK(hipSetDevice(c->device));
        HCHECK(hipStreamSynchronize(c->stream));
        if (n > 0 && state) HCHECK(hipMemcpy(state, M.d_state.p, (size_t)n, hipMemcpyDeviceToHost));
        if (n > 0 && bases) HCHECK(hipMemcpy(bases, M.d_bases.p, (size_t)n * 2, hipMemcpyDeviceToHost));
        return HIMUT_OK;
    });
}

}  // extern "C"
