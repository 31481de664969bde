// libhimut_hip.so: the dbs run (himut_run_dbs, himut_get_dbs) over the kernels of himut_dbs.h.  Its front half -- the cs
// decode, the column index, the capture -- is the column front it shares with the call and germline runs (front_plan,
// front_decode, front_capture: himut_call.hip), without proposals; its back end -- the scalars' copy-back, the state left
// for the next run, the stage times -- is the front's too (front_tail, front_stats).
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

// the number of keys k_dbs_propose wanted to append (the host waits for the stream)
int64_t read_nprop(himut_ctx* c) {
    unsigned long long n = 0;
    HCHECK(hipMemcpyAsync(&n, c->dbs.d_sc.as<unsigned long long>() + DBS_SC_NPROP, 8, hipMemcpyDeviceToHost, c->stream));
    HCHECK(hipStreamSynchronize(c->stream));
    return (int64_t)n;
}

void reserve_for_keys(himut_ctx* c, int64_t cap_props) {
    himut_ctx::Dbs& B = c->dbs;
    const unsigned nwg = blocks_for(cap_props, 256);
    B.d_keys.reserve((size_t)cap_props * 8 + 256);
    B.d_keys2.reserve((size_t)cap_props * 8 + 256);
    B.d_recs.reserve(((size_t)nwg * 256 + 1) * sizeof(himut_dbs_record));
    B.d_recs_out.reserve(((size_t)nwg * 256 + 1) * sizeof(himut_dbs_record));
    B.d_wgcnt.reserve((size_t)nwg * 4 + 64);
    if (cap_props > 0) {
        size_t tmp = 0;
        HCHECK(rocprim::radix_sort_keys(nullptr, tmp, B.d_keys.as<uint64_t>(), B.d_keys2.as<uint64_t>(), (size_t)cap_props, 0, 40, c->stream));
        B.d_sorttmp.reserve(tmp + 256);
    }
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
    if (int rc = front_capture(c, &F, C, make_phase(c), P, nullptr, nullptr)) return rc;      // no proposals
    Scalars* sc = c->d_scalars.as<Scalars>();

    int64_t cap_props = spec ? B.cap_props : 0, nprop = 0;
    bool props_over = false;
    if (c->n > 0) {
        if (!spec) {
            // the count first (nothing is written with no capacity), then the buffers with 25 % of headroom for the runs that follow
            launch_propose(c, P, T.n, 0, sc);
            nprop = read_nprop(c);
            cap_props = nprop + nprop / 4 + 1024;
            reserve_for_keys(c, cap_props);
        }
        launch_propose(c, P, T.n, cap_props, sc);
        nprop = read_nprop(c);
        props_over = nprop > cap_props;                  // only a run on kept capacities can get here
        unsigned long long* dsc = B.d_sc.as<unsigned long long>();
        if (!props_over && nprop > 0) {
            size_t tmp = 0;                              // (the sort of fewer keys may want more room than the sort of the capacity)
            HCHECK(rocprim::radix_sort_keys(nullptr, tmp, B.d_keys.as<uint64_t>(), B.d_keys2.as<uint64_t>(), (size_t)nprop, 0, 40, st));
            B.d_sorttmp.reserve(tmp + 256);
            HCHECK(rocprim::radix_sort_keys(B.d_sorttmp.p, tmp, B.d_keys.as<uint64_t>(), B.d_keys2.as<uint64_t>(), (size_t)nprop, 0, 40, st));
            const unsigned nwg = blocks_for(nprop, 256);
            DbsArgs A;
            A.P = P; A.S = site_sets(c); A.lut = c->d_lut.as<GtLut>(); A.X = F.X;
            A.colstore = c->call.d_colstore.as<uint16_t>(); A.nslots = (int64_t)F.slot_cap;
            A.keys = B.d_keys2.as<uint64_t>(); A.nkeys = nprop;
            A.recs = B.d_recs.as<himut_dbs_record>(); A.wgcnt = B.d_wgcnt.as<uint32_t>(); A.sc = dsc; A.err = &sc->err;
            hipLaunchKernelGGL(k_dbs_eval, dim3(nwg), dim3(256), 0, st, A);
            stage_event(c, EV_SWEEP, 2, st);
            hipLaunchKernelGGL((k_compact_runs<himut_dbs_record, DbsRuns>), dim3(nwg), dim3(256), 0, st, B.d_wgcnt.as<uint32_t>(),
                               DbsRuns{B.d_recs.as<himut_dbs_record>()}, B.d_recs_out.as<himut_dbs_record>(), dsc + DBS_SC_NREC);
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
    if (props_over || nslots > (int64_t)F.slot_cap) {
        *overflow = true;
        return HIMUT_OK;
    }
    if (!spec && c->n > 0) { B.cap_props = cap_props; B.cap_slots = kept_slot_cap(F.slot_cap); }
    B.out.n = (int64_t)hsc[DBS_SC_NREC];
    take_log(B.out, hsc + DBS_SC_LOG);

    front_stats(c, EVAL_STAGES, N_EVAL_STAGES, T.positions, nprop, B.out.n, nslots);
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
