// libhimut_hip.so: the support run (himut_run_support, himut_get_support) over the kernels of himut_support.h.  The cs
// decode in front of it is the read pass every pipeline starts with (run_parse_stage, himut_front.hip), under a
// parameter block of the run's own.
#include <hip/hip_runtime.h>

#include "himut_ctx.h"
#include "himut_support.h"

using namespace himut;

extern "C" {

int himut_run_support(himut_ctx* c, const int32_t* pos1, const uint8_t* ref, const uint8_t* alt, int64_t n_sites,
                      const himut_support_params* p) {
    if (!c) return HIMUT_ERR_ARG;
    if (!p || n_sites < 0 || n_sites > INT32_MAX || (n_sites && (!pos1 || !ref || !alt))) return fail(c, HIMUT_ERR_ARG, "himut_run_support: bad argument");
    return guarded(c, [&]() -> int {
        if (int rc = check_run_inputs(c, NEED_READS)) return rc;
        if (p->mismatch_window_size < 0) return fail(c, HIMUT_ERR_ARG, "himut_run_support: negative mismatch window");
        std::vector<uint8_t> code;
        if (int rc = encode_sites(c, "himut_run_support", pos1, ref, alt, n_sites, &code)) return rc;
        HCHECK(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        himut_ctx::Support& S = c->support;
        S.n_rows = 0; S.n_sites = n_sites;
        S.h_rows.clear();
        S.h_counts.assign((size_t)n_sites * 2, 0);
        memset(&c->stats, 0, sizeof(c->stats));

        alloc_derived(c);
        const size_t ns1 = (size_t)n_sites + 1;
        S.d_counts.reserve(ns1 * 8);
        S.d_rowoff.reserve((ns1 + 1) * 8);
        S.d_cursor.reserve(ns1 * 4);
        S.d_sc.reserve(sizeof(Scalars));
        upload(S.d_pos, pos1, (size_t)n_sites, st);
        upload(S.d_code, code.data(), (size_t)n_sites, st);
        Scalars* sc = S.d_sc.as<Scalars>();        // (not the context's: the call and germline runs keep theirs as they left them)
        Scalars hs;
        memset(&hs, 0, sizeof(hs));

        HCHECK(hipEventRecord(c->ev[EV_START], st));
        HCHECK(hipMemsetAsync(sc, 0, sizeof(Scalars), st));
        HCHECK(hipMemsetAsync(S.d_counts.p, 0, ns1 * 8, st));
        HCHECK(hipMemsetAsync(S.d_cursor.p, 0, ns1 * 4, st));
        // the decode marks nothing (no bitmap) and flags every read's identity as passing: query-length limits open, identity -1
        const Params P = open_gate_params(c, p->min_mapq);
        SupportArgs A;
        A.R = make_reads(c); A.D = make_derived(c);
        A.pos1 = S.d_pos.as<int32_t>(); A.code = S.d_code.as<uint8_t>(); A.nsites = n_sites;
        A.min_mapq = p->min_mapq; A.window = p->mismatch_window_size;
        A.counts = S.d_counts.as<int32_t>(); A.rowoff = S.d_rowoff.as<int64_t>(); A.cursor = S.d_cursor.as<uint32_t>();
        A.rows = nullptr;
        const bool work = c->n > 0 && n_sites > 0;
        if (c->n > 0) run_parse_stage(c, A.R, A.D, sc, &P);
        else stage_event(c, EV_PARSE, 2, st);
        if (work) hipLaunchKernelGGL(k_support<false>, dim3(blocks_for(c->n, 4)), dim3(256), 0, st, A);
        hipLaunchKernelGGL(k_support_scan, dim3(1), dim3(256), 0, st, S.d_counts.as<int32_t>(), n_sites, S.d_rowoff.as<int64_t>(), &sc->nrec);
        stage_event(c, EV_INDEX, 2, st);
        HCHECK(hipMemcpyAsync(&hs, sc, sizeof(Scalars), hipMemcpyDeviceToHost, st));
        HCHECK(hipStreamSynchronize(st));
        if (hs.err) return check_device_err(c, hs.err);
        const int64_t nrows = (int64_t)hs.nrec;
        if (nrows > 0) {
            S.d_rows_in.reserve((size_t)nrows * sizeof(himut_support_row));
            S.d_rows.reserve((size_t)nrows * sizeof(himut_support_row));
            A.rows = S.d_rows_in.as<himut_support_row>();
            hipLaunchKernelGGL(k_support<true>, dim3(blocks_for(c->n, 4)), dim3(256), 0, st, A);
            stage_event(c, EV_GATHER, 2, st);
            hipLaunchKernelGGL(k_support_order, dim3(blocks_for(nrows, 256)), dim3(256), 0, st, S.d_rows_in.as<himut_support_row>(),
                               S.d_rowoff.as<int64_t>(), n_sites, nrows, S.d_rows.as<himut_support_row>());
        } else {
            stage_event(c, EV_GATHER, 2, st);
        }
        HCHECK(hipEventRecord(c->ev[EV_FINAL], st));
        S.h_rows.resize((size_t)nrows);
        if (nrows) HCHECK(hipMemcpyAsync(S.h_rows.data(), S.d_rows.p, (size_t)nrows * sizeof(himut_support_row), hipMemcpyDeviceToHost, st));
        if (n_sites) HCHECK(hipMemcpyAsync(S.h_counts.data(), S.d_counts.p, (size_t)n_sites * 8, hipMemcpyDeviceToHost, st));
        HCHECK(hipStreamSynchronize(st));
        S.n_rows = nrows;
        c->stats.ms_total = elapsed_ms(c, EV_START, EV_FINAL);
        if (c->timing >= 2) {       // the count pass and the scan, the fill pass, the ordering (the host reads the row total in between)
            c->stats.ms_parse = elapsed_ms(c, EV_START, EV_PARSE);
            c->stats.ms_index = elapsed_ms(c, EV_PARSE, EV_INDEX);
            c->stats.ms_capture = elapsed_ms(c, EV_INDEX, EV_GATHER);
            c->stats.ms_finalize = elapsed_ms(c, EV_GATHER, EV_FINAL);
        }
        c->stats.n_reads = c->n; c->stats.read_bases = c->read_bases; c->stats.n_records = nrows;
        return HIMUT_OK;
    });
}

int himut_get_support(himut_ctx* c, const himut_support_row** rows, int64_t* n_rows, const int32_t** site_counts) {
    if (!c || !rows || !n_rows) return HIMUT_ERR_ARG;
    const himut_ctx::Support& S = c->support;
    *rows = S.h_rows.data();
    *n_rows = S.n_rows;
    if (site_counts) *site_counts = S.h_counts.data();
    return HIMUT_OK;
}

}  // extern "C"
