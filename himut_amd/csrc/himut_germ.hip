// libhimut_hip.so: the germline run (himut_run_germline, himut_get_germline) over the kernels of himut_germ.h.  Its
// front half -- the cs decode, the column index, the capture -- is the column front it shares with the call run
// (front_plan, front_decode, front_capture: himut_front.hip), without proposals and with nothing between the steps; its
// back end -- the copy-back, the state left for the next run, the stage times -- is the front's too (front_tail, front_stats).
#include <hip/hip_runtime.h>

#include "himut_ctx.h"
#include "himut_germ.h"

using namespace himut;

namespace {

// One pass.  spec: the buffers keep the capacities of the previous germline run and the host waits for nothing in the
// middle; *overflow is set if the marked positions or the column slots did not fit (the caller runs again with exact sizes).
int germ_once(himut_ctx* c, const himut_germline_params& gp, bool allow_spec, bool* overflow) {
    *overflow = false;
    if (int rc = check_run_inputs(c, NEED_LUT | NEED_READS | NEED_REGIONS | NEED_SPANS)) return rc;
    himut_ctx::Germ& G = c->germ;
    begin_run(c, G.out);
    hipStream_t st = c->stream;

    ChunkTables T = upload_chunks(c, c->cstart, c->cend);
    alloc_derived(c);
    Chunks C = make_chunks(c, T.n);
    // every pile read marks its substitutions: the germline min_mapq, the other gates of the bitmap open
    const Params P = open_gate_params(c, gp.min_mapq);
    const bool spec = allow_spec && G.cap_marked > 0 && G.cap_slots > 0 && c->n > 0;
    ColumnFront F = front_plan(c, spec, G.cap_slots);
    front_decode(c, F, P, false);
    if (int rc = front_capture(c, &F, C, make_phase(c), P, Proposals::none)) return rc;
    Scalars* sc = c->d_scalars.as<Scalars>();

    const int64_t cap_marked = spec ? G.cap_marked : F.marked + F.marked / 4 + 1024;
    const unsigned nwg = blocks_for(F.nblk, GERM_WG_BLOCKS);
    if (c->n > 0) {
        G.d_refmask.reserve((size_t)cap_marked + 256);
        G.d_nrefbits.reserve(F.lead_bytes + 256);
        G.d_recs.reserve((size_t)(cap_marked + 1) * sizeof(himut_record));
        G.d_recs_out.reserve((size_t)(cap_marked + 1) * sizeof(himut_record));
        G.d_wgcnt.reserve((size_t)nwg * 4 + 64);
        G.d_logpart.reserve((size_t)nwg * 12 * 4 + 64);
        HCHECK(hipMemsetAsync(G.d_refmask.p, 0, ((size_t)cap_marked + 3) & ~(size_t)3, st));
        HCHECK(hipMemsetAsync(G.d_nrefbits.p, 0, F.lead_bytes, st));
        hipLaunchKernelGGL(k_germ_refbase, dim3(blocks_for(c->n, 16)), dim3(256), 0, st, make_reads(c), make_derived(c), F.X, (int)gp.min_mapq,
                           G.d_refmask.as<uint32_t>(), cap_marked, G.d_nrefbits.as<uint32_t>(), &sc->err);
        GermArgs A;
        A.p = gp; A.lut = c->d_lut.as<GtLut>(); A.R = make_reads(c); A.D = make_derived(c); A.X = F.X;
        A.s_start = c->d_sstart.as<int32_t>(); A.s_pmaxend = c->d_spmax.as<int32_t>(); A.nregion = T.n;
        A.colstore = c->call.d_colstore.as<uint16_t>(); A.nslots = (int64_t)F.slot_cap;
        A.refmask = G.d_refmask.as<uint32_t>(); A.nrefbits = G.d_nrefbits.as<uint32_t>(); A.cap_marked = cap_marked;
        A.recs = G.d_recs.as<himut_record>(); A.wgcnt = G.d_wgcnt.as<uint32_t>(); A.logpart = G.d_logpart.as<uint32_t>();
        A.err = &sc->err;
        hipLaunchKernelGGL(gp.min_mapq > 0 ? k_germline_eval<true> : k_germline_eval<false>, dim3(nwg), dim3(256), 0, st, A);
        stage_event(c, EV_SWEEP, 2, st);
        const GermRuns runs{G.d_recs.as<himut_record>(), G.d_logpart.as<uint32_t>(), c->call.d_blkoff.as<uint32_t>(),
                            c->call.d_blkslots.as<uint32_t>(), F.X, cap_marked, &sc->ncand, &sc->nslots, sc->log};
        hipLaunchKernelGGL((k_compact_runs<himut_record, GermRuns>), dim3(nwg), dim3(256), 0, st, G.d_wgcnt.as<uint32_t>(), runs,
                           G.d_recs_out.as<himut_record>(), &sc->nrec);
    } else {
        stage_event(c, EV_SWEEP, 2, st);
    }
    front_tail(c, F);                                    // (leaves the front empty for the next run, of this kind or the call run's)
    if (int rc = front_tail_wait(c, F)) return rc;
    const Scalars& hs = *reinterpret_cast<const Scalars*>(c->h_scalars);
    const int64_t marked = c->n > 0 ? (int64_t)hs.ncand : 0, nslots = c->n > 0 ? (int64_t)hs.nslots : 0;
    if (marked > cap_marked || nslots > (int64_t)F.slot_cap) {       // only a run on kept capacities can get here
        *overflow = true;
        return HIMUT_OK;
    }
    if (!spec && c->n > 0) { G.cap_marked = cap_marked; G.cap_slots = kept_slot_cap(F.slot_cap); }
    if (c->n > 0) { G.out.n = (int64_t)hs.nrec; take_log(G.out, hs.log); }

    front_stats(c, EVAL_STAGES, N_EVAL_STAGES, T.positions, marked, G.out.n, nslots);
    return HIMUT_OK;
}

}  // namespace

extern "C" {

int himut_run_germline(himut_ctx* c, const himut_germline_params* p) {
    if (!c || !p) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int {
        return run_repeating(c, [&](bool kept, bool* overflow) { return germ_once(c, *p, kept, overflow); },
                             [&] { c->germ.cap_marked = c->germ.cap_slots = 0; });
    });
}

int himut_get_germline(himut_ctx* c, const himut_record** records, int64_t* n, int64_t log[12]) {
    if (!c || !records || !n) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int { return get_run_out(c, c->germ.out, c->germ.d_recs_out, records, n, log); });
}

}  // extern "C"
