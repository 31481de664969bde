// libhimut_hip.so: the sites run (himut_run_sites, himut_get_sites) over the kernels of himut_sites.h.  It goes over the
// column front of the call, germline and dbs runs (front_plan, front_decode, front_capture: himut_front.hip) with the
// bitmap filled from the host's site list instead of from the reads; its back end -- the scalars' copy-back, the state
// left for the next run, the stage times -- is the front's too (front_tail, front_stats).  The pass is two steps
// (sites_front, sites_back: himut_ctx.h) on one set of buffers, so that the duplex run, whose sites come from the decoded
// reads, takes the same pass on buffers of its own.
#include <hip/hip_runtime.h>

#include "himut_ctx.h"
#include "himut_sites.h"

using namespace himut;

namespace himut {

SitesFront sites_front(himut_ctx* c, SitesBufs& B, const Params& decode, bool allow_spec) {
    alloc_derived(c);
    B.d_sc.reserve(SITES_SC_WORDS * 8);
    SitesFront SF;
    SF.decode = decode;
    SF.spec = allow_spec && B.cap_slots > 0 && c->n > 0;
    SF.F = front_plan(c, SF.spec, B.cap_slots, false);               // regions do not exist: the reads' span alone
    front_decode(c, SF.F, SF.decode, false);
    return SF;
}

int sites_back(himut_ctx* c, SitesBufs& B, SitesFront& SF, int64_t n_sites, bool* overflow, SitesTotals* out) {
    *overflow = false;
    hipStream_t st = c->stream;
    ColumnFront& F = SF.F;
    // the evaluation reads the call run's thresholds; phased lookups are out of scope
    Params P = c->params;
    P.p.phase = 0;
    if (c->n > 0 && n_sites > 0)
        hipLaunchKernelGGL(k_sites_mark, dim3(blocks_for(n_sites, 256)), dim3(256), 0, st, B.d_pos.as<int32_t>(), n_sites,
                           c->call.d_posbits_c.as<uint32_t>(), F.nwords);
    Chunks C{};                                                       // an empty region table: the capture's tail check cannot fire
    if (int rc = front_capture(c, &F, C, make_phase(c), SF.decode, Proposals::none)) return rc;
    Scalars* sc = c->d_scalars.as<Scalars>();

    unsigned long long* dsc = B.d_sc.as<unsigned long long>();
    HCHECK(hipMemsetAsync(dsc, 0, SITES_SC_WORDS * 8, st));
    if (n_sites > 0) {
        SitesArgs A;
        A.P = P; A.S = site_sets(c); A.lut = c->d_lut.as<GtLut>(); A.X = F.X;
        if (c->n <= 0) A.X.nwords = 0;                                // no reads: no index was built, no site has a column
        A.colstore = c->call.d_colstore.as<uint16_t>(); A.nslots = (int64_t)F.slot_cap;
        A.mapq = c->d_mapq.as<uint8_t>();
        A.pos1 = B.d_pos.as<int32_t>(); A.code = B.d_code.as<uint8_t>(); A.nsites = n_sites;
        A.recs = B.d_recs.as<himut_site_record>(); A.sc = dsc; A.err = &sc->err;
        hipLaunchKernelGGL(k_sites_eval, dim3(blocks_for(n_sites, 256)), dim3(256), 0, st, A);
    }
    stage_event(c, EV_SWEEP, 2, st);
    if (c->n > 0) front_totals(c, F, dsc, SITES_SC_LOG + SITES_LOG_MARKED, SITES_SC_NSLOTS);
    front_tail(c, F);                                    // (leaves the front empty for the next run over it, of any kind)
    if (int rc = front_tail_wait(c, F)) return rc;
    unsigned long long hsc[SITES_SC_WORDS] = {};         // the pass's own scalars: nothing of the tail touches them
    HCHECK(hipMemcpyAsync(hsc, dsc, sizeof(hsc), hipMemcpyDeviceToHost, st));
    HCHECK(hipStreamSynchronize(st));
    out->nslots = (int64_t)hsc[SITES_SC_NSLOTS];
    if (out->nslots > (int64_t)F.slot_cap) {             // only a pass on kept capacities can get here
        *overflow = true;
        return HIMUT_OK;
    }
    if (!SF.spec && c->n > 0) B.cap_slots = kept_slot_cap(F.slot_cap);
    for (int k = 0; k < 20; k++) out->log[k] = (int64_t)hsc[SITES_SC_LOG + k];
    return HIMUT_OK;
}

}  // namespace himut

namespace {

// One pass over the sites in S.d_pos / S.d_code.  kept: the column store keeps the capacity of the previous sites run
// and the host waits for nothing in the middle; *overflow is set if the column slots did not fit (the caller runs again
// with exact sizes).
int sites_once(himut_ctx* c, int64_t n_sites, bool allow_spec, bool* overflow) {
    *overflow = false;
    himut_ctx::Sites& S = c->sites;
    begin_run(c, S.out);
    // the decode's own block: closed query-length limits, so no read passes the bitmap gate and the decode marks nothing
    Params PD = open_gate_params(c, 0);
    PD.p.qlen_lower_limit = INT_MAX; PD.p.qlen_upper_limit = -1;
    SitesFront SF = sites_front(c, S, PD, allow_spec);
    SitesTotals T;
    if (int rc = sites_back(c, S, SF, n_sites, overflow, &T)) return rc;
    if (*overflow) return HIMUT_OK;
    S.out.n = n_sites;
    take_log(S.out, T.log);

    front_stats(c, EVAL_STAGES, N_EVAL_STAGES, 0, n_sites, n_sites, T.nslots);
    return HIMUT_OK;
}

}  // namespace

extern "C" {

int himut_run_sites(himut_ctx* c, const int32_t* pos1, const uint8_t* ref, const uint8_t* alt, int64_t n_sites) {
    if (!c) return HIMUT_ERR_ARG;
    if (n_sites < 0 || n_sites > INT32_MAX || (n_sites && (!pos1 || !ref || !alt))) return fail(c, HIMUT_ERR_ARG, "himut_run_sites: bad argument");
    return guarded(c, [&]() -> int {
        if (int rc = check_run_inputs(c, NEED_PARAMS | NEED_LUT | NEED_READS)) return rc;
        std::vector<uint8_t> code;
        if (int rc = encode_sites(c, "himut_run_sites", pos1, ref, alt, n_sites, &code)) return rc;
        himut_ctx::Sites& S = c->sites;
        begin_run(c, S.out);                             // (the buffers below may move: what the getter served is gone)
        // the run's own buffers, before anything of it is queued (DevBuf::reserve drains the device when it grows)
        S.d_recs.reserve(((size_t)n_sites + 1) * sizeof(himut_site_record));
        S.d_sc.reserve(SITES_SC_WORDS * 8);
        upload(S.d_pos, pos1, (size_t)n_sites, c->stream);
        upload(S.d_code, code.data(), (size_t)n_sites, c->stream);
        HCHECK(hipStreamSynchronize(c->stream));         // (code is a local: its copy must be over before it goes)
        return run_repeating(c, [&](bool kept, bool* overflow) { return sites_once(c, n_sites, kept, overflow); },
                             [&] { c->sites.cap_slots = 0; });
    });
}

int himut_get_sites(himut_ctx* c, const himut_site_record** records, int64_t* n, int64_t log[20]) {
    if (!c || !records || !n) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int { return get_run_out(c, c->sites.out, c->sites.d_recs, records, n, log); });
}

}  // extern "C"
