// libhimut_hip.so: the dbs run (himut_run_dbs, himut_get_dbs) over the kernels of himut_dbs.h.  Its front half -- the cs
// decode, the column index, the capture -- is the column front it shares with the call and germline runs (front_plan,
// front_decode, front_capture: himut_front.hip), without proposals; its back end -- the scalars' copy-back, the state left
// for the next run, the stage times -- is the front's too (front_tail, front_stats).  Between them the proposals are a
// counted key list (count_keys, sort_with_tmp: himut_ctx.h, as the indels run's events).
#include <hip/hip_runtime.h>

#include <string.h>  // rocprim's texture iterator needs the host memset declared first
#include <rocprim/rocprim.hpp>

#include "himut_ctx.h"
#include "himut_dbs.h"

using namespace himut;

namespace {

void launch_propose(himut_ctx* c, const Params& P, int64_t nregion, int64_t cap_props, Scalars* sc) {
    himut_ctx::Dbs& B = c->dbs;
    HCHECK(hipMemsetAsync(B.d_sc.p, 0, DBS_SC_WORDS * 8, c->stream));
    hipLaunchKernelGGL(k_dbs_propose, dim3(blocks_for(c->n, 16)), dim3(256), 0, c->stream, make_reads(c), make_derived(c), P,
                       c->d_sstart.as<int32_t>(), c->d_spmax.as<int32_t>(), nregion, B.d_keys.as<uint64_t>(), cap_props,
                       B.d_sc.as<unsigned long long>(), &sc->err);
}

// rocPRIM's sort of the first n keys (40 bits: himut_dbs.h) from d_keys into d_keys2; tmp null: the temporary size alone
hipError_t sort_keys(himut_ctx* c, void* tmp, size_t& bytes, int64_t n) {
    himut_ctx::Dbs& B = c->dbs;
    return rocprim::radix_sort_keys(tmp, bytes, B.d_keys.as<uint64_t>(), B.d_keys2.as<uint64_t>(), (size_t)n, 0, 40, c->stream);
}

void reserve_for_keys(himut_ctx* c, int64_t cap_props) {
    himut_ctx::Dbs& B = c->dbs;
    const unsigned nwg = blocks_for(cap_props, 256);
    B.d_keys.reserve((size_t)cap_props * 8 + 256);
    B.d_keys2.reserve((size_t)cap_props * 8 + 256);
    B.d_recs.reserve(((size_t)nwg * 256 + 1) * sizeof(himut_dbs_record));
    B.d_recs_out.reserve(((size_t)nwg * 256 + 1) * sizeof(himut_dbs_record));
    B.d_wgcnt.reserve((size_t)nwg * 4 + 64);
    if (cap_props > 0) sort_with_tmp(B.d_sorttmp, false, [&](void* tmp, size_t& bytes) { return sort_keys(c, tmp, bytes, cap_props); });
}

// One pass.  kept: the key and column-store buffers keep the capacities of the previous dbs run; *overflow is set if the
// proposals or the column slots did not fit (the caller runs again with exact sizes).  The host waits once in the
// middle, for the number of proposals (the sort and the grids behind it take it).
int dbs_once(himut_ctx* c, bool allow_spec, bool* overflow) {
    *overflow = false;
    if (int rc = check_run_inputs(c, NEED_PARAMS | NEED_LUT | NEED_READS | NEED_REGIONS | NEED_SPANS)) return rc;
    himut_ctx::Dbs& B = c->dbs;
    begin_run(c, B.out);
    hipStream_t st = c->stream;

    ChunkTables T = upload_chunks(c, c->cstart, c->cend);
    alloc_derived(c);
    Chunks C = make_chunks(c, T.n);
    // the call run's parameter block: the bitmap holds the substitutions of the reads that pass its mapq, query-length
    // and identity gates, a superset of the proposing reads'; phased doublet calling is out of scope
    Params P = c->params;
    P.p.phase = 0;
    const bool spec = allow_spec && B.cap_props > 0 && B.cap_slots > 0 && c->n > 0;
    ColumnFront F = front_plan(c, spec, B.cap_slots);
    B.d_sc.reserve(DBS_SC_WORDS * 8);
    if (spec) reserve_for_keys(c, B.cap_props);
    front_decode(c, F, P, false);
    if (int rc = front_capture(c, &F, C, make_phase(c), P, Proposals::none)) return rc;
    Scalars* sc = c->d_scalars.as<Scalars>();

    KeyCount K{0, 0, false};                             // the proposals: their number, the capacity they had, whether it held them
    if (c->n > 0) {
        unsigned long long* dsc = B.d_sc.as<unsigned long long>();
        K = count_keys(c, spec, B.cap_props, dsc + DBS_SC_NPROP, [&](int64_t cap) { launch_propose(c, P, T.n, cap, sc); },
                       [&](int64_t cap) { reserve_for_keys(c, cap); });
        const int64_t nprop = K.n;
        if (!K.over && nprop > 0) {
            sort_with_tmp(B.d_sorttmp, true, [&](void* tmp, size_t& bytes) { return sort_keys(c, tmp, bytes, nprop); });
            const unsigned nwg = blocks_for(nprop, 256);
            DbsArgs A;
            A.P = P; A.S = site_sets(c); A.lut = c->d_lut.as<GtLut>(); A.X = F.X;
            A.colstore = c->call.d_colstore.as<uint16_t>(); A.nslots = (int64_t)F.slot_cap;
            A.keys = B.d_keys2.as<uint64_t>(); A.nkeys = nprop;
            A.recs = B.d_recs.as<himut_dbs_record>(); A.wgcnt = B.d_wgcnt.as<uint32_t>(); A.sc = dsc; A.err = &sc->err;
            hipLaunchKernelGGL(k_dbs_eval, dim3(nwg), dim3(256), 0, st, A);
            stage_event(c, EV_SWEEP, 2, st);
            hipLaunchKernelGGL((k_compact_runs<himut_dbs_record, SlotRuns<himut_dbs_record>>), dim3(nwg), dim3(256), 0, st, B.d_wgcnt.as<uint32_t>(),
                               SlotRuns<himut_dbs_record>{B.d_recs.as<himut_dbs_record>()}, B.d_recs_out.as<himut_dbs_record>(), dsc + DBS_SC_NREC);
        } else {
            stage_event(c, EV_SWEEP, 2, st);
        }
        front_totals(c, F, dsc, DBS_SC_NMARKED, DBS_SC_NSLOTS);
    } else {
        stage_event(c, EV_SWEEP, 2, st);
    }
    front_tail(c, F);                                    // (leaves the front empty for the next run over it, of any kind)
    if (int rc = front_tail_wait(c, F)) return rc;
    unsigned long long hsc[DBS_SC_WORDS] = {};           // the run's own scalars: nothing of the tail touches them
    if (c->n > 0) {
        HCHECK(hipMemcpyAsync(hsc, B.d_sc.p, sizeof(hsc), hipMemcpyDeviceToHost, st));
        HCHECK(hipStreamSynchronize(st));
    }
    const int64_t nslots = (int64_t)hsc[DBS_SC_NSLOTS];
    if (K.over || nslots > (int64_t)F.slot_cap) {
        *overflow = true;
        return HIMUT_OK;
    }
    if (!spec && c->n > 0) { B.cap_props = K.cap; B.cap_slots = kept_slot_cap(F.slot_cap); }
    B.out.n = (int64_t)hsc[DBS_SC_NREC];
    take_log(B.out, hsc + DBS_SC_LOG);

    front_stats(c, EVAL_STAGES, N_EVAL_STAGES, T.positions, K.n, B.out.n, nslots);
    return HIMUT_OK;
}

}  // namespace

extern "C" {

int himut_run_dbs(himut_ctx* c) {
    if (!c) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int {
        return run_repeating(c, [&](bool kept, bool* overflow) { return dbs_once(c, kept, overflow); },
                             [&] { c->dbs.cap_props = c->dbs.cap_slots = 0; });
    });
}

int himut_get_dbs(himut_ctx* c, const himut_dbs_record** records, int64_t* n, int64_t log[20]) {
    if (!c || !records || !n) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int { return get_run_out(c, c->dbs.out, c->dbs.d_recs_out, records, n, log); });
}

}  // extern "C"
