// libhimut_hip.so: the call run (himut_run, himut_run_begin / _end) behind the column front (himut_front.hip), over the
// kernels of himut_call.h as a sequence of steps (call_plan, call_candidates, call_eval, call_finalize, finish_run); its
// records and counters.
#include <hip/hip_runtime.h>

#include <string.h>  // rocprim's texture iterator needs the host memset declared first
#include <rocprim/rocprim.hpp>

#include "himut_ctx.h"
#include "himut_call.h"

using namespace himut;

namespace {

// One pass of the call run (do_run_once): call_plan -> the column front, k_read_hap between its decode and its capture
// -> call_candidates -> call_eval -> call_finalize -> the front's tail.  spec: the candidate and column-slot buffers keep
// the capacities of an earlier run (cap_cand, cap_slots) and every kernel behind a count takes the count from device
// memory, so the host launches the whole run without waiting in the middle; *overflow is set if a count did not fit (the
// caller runs again with exact sizes).  Otherwise the host waits for the counts where it needs them (front_capture,
// call_candidates) and sizes the buffers with 25 % of headroom for the runs that follow.

// The buffers the candidate count sizes, all of them and nowhere else: from call_plan on kept capacities, else once,
// behind the count's read-back in call_candidates (nothing is queued on them yet, and the stream has just been waited
// for).  A run on kept capacities reserves nothing behind EV_START.
void call_reserve_records(himut_ctx* c, CallPlan* P) {
    himut_ctx::Call& K = c->call;
    const int64_t nreserve = P->nreserve;
    K.d_recs.reserve((size_t)(nreserve + 1) * sizeof(himut_record));
    K.d_recs_out.reserve((size_t)(nreserve + 1) * sizeof(himut_record));
    if (P->ncap <= 0) return;
    K.d_keys.reserve((size_t)nreserve * 8); K.d_keys2.reserve((size_t)nreserve * 8);
    K.d_cands.reserve((size_t)nreserve * sizeof(Cand) + 256); K.d_cands2.reserve((size_t)nreserve * sizeof(Cand) + 256);
    K.d_emit.reserve((size_t)nreserve * 4);
    if (!c->chunks_in_order) {                               // the sort into the order of the final records
        HCHECK(rocprim::radix_sort_pairs(nullptr, P->sort_tmp, K.d_keys.as<uint64_t>(), K.d_keys2.as<uint64_t>(), K.d_cands.as<uint64_t>(),
                                         K.d_cands2.as<uint64_t>(), (size_t)P->ncap, 0, 60, c->stream));
        c->d_tmp.reserve(P->sort_tmp + 256);
    }
    const unsigned nb = blocks_for(P->ncap, 256);            // the finalisation's workgroups
    K.d_logpart.reserve((size_t)nb * 16 * 4 + 64);
    K.d_pos.reserve((size_t)nb * 4 + 64);                    // where each workgroup's emitted records begin
}

// Everything the host knows before anything of the run is queued, and every buffer whose size it knows by then
// reserved: DevBuf::reserve drains the device when it grows, and growing a buffer in the middle of a run would free it
// under the kernels already queued on it.
int call_plan(himut_ctx* c, bool allow_spec, CallPlan* P) {
    himut_ctx::Call& K = c->call;
    P->T = upload_chunks(c, c->cstart, c->cend);
    P->phase = c->params.p.phase != 0;
    // the sorted-chunk path writes the candidates in their final order straight from the mask: only that one
    // has nothing between the count and its consumers that needs the count on the host
    P->spec = allow_spec && c->chunks_in_order && K.cap_cand > 0 && K.cap_slots > 0 && P->T.positions > 0 && c->n > 0;
    alloc_derived(c);
    P->F = front_plan(c, P->spec, K.cap_slots);
    // The mask.  Chunks in order: a 16-bit cell per (marked position, chunk) by column rank, sized with the column store --
    // here on kept capacities, else behind the host's read-back in front_capture; its tiles are the workgroups of the
    // column index.  Any other list: a cell per (chunk, position), in tiles of 8192.  One buffer serves both: whichever
    // way a run indexed it, its emit leaves it zeroed.
    P->by_rank = c->chunks_in_order;
    const uint64_t mask_was = K.d_mask.gen;
    if (P->by_rank) {
        P->mtiles = P->F.idx_wgs;
        if (P->spec) {
            P->F.rmask_cells = K.cap_slots + P->T.n;
            K.d_mask.reserve(rank_mask_bytes((size_t)K.cap_slots, P->T.n));
        }
    } else {
        P->n4 = ((int64_t)P->T.positions * 2 + 15) / 16;
        P->mask_bytes = (size_t)P->n4 * 16;
        P->anyw = ((int64_t)P->T.positions + 31) / 32;
        P->mtiles = blocks_for(P->anyw, 256);
        K.d_mask.reserve(P->mask_bytes + 64);
    }
    // the emit zeroes what the proposals set: a buffer that went through a whole run is clean
    const bool clear_mask = !K.mask_clean || mask_was != K.d_mask.gen;
    K.mask_clean = false;
    const uint64_t tcnt_was = K.d_tilecnt.gen;
    K.d_tilecnt.reserve((size_t)P->mtiles * 4 + 64);
    K.d_tileoff2.reserve((size_t)P->mtiles * 4 + 64);
    P->clear_all = clear_mask || tcnt_was != K.d_tilecnt.gen;
    if (P->phase && P->T.n > 65535) return fail(c, HIMUT_ERR_ARG, "--phase: more than 65,535 chunks in one contig (k_read_hap takes a chunk per grid row)");
    if (P->phase) c->d_hap.reserve((size_t)P->T.npairs + 64);
    if (P->mtiles > 65536u) {                                          // (else one workgroup scans the tile counts: k_scan_small)
        uint32_t* nul = nullptr;
        HCHECK(rocprim::exclusive_scan(nullptr, P->scan_tiles, nul, nul, 0u, (size_t)P->mtiles, rocprim::plus<uint32_t>(), c->stream));
    }
    c->d_tmp2.reserve(P->scan_tiles + 256);
    if (P->spec) {
        P->ncap = P->nreserve = K.cap_cand;
        call_reserve_records(c, P);
    }
    return HIMUT_OK;
}

// .. EV_EMIT: the candidates = the set bits of the mask.  Chunks in order: k_mask_count counts them per tile, k_mask_emit
// places its tiles itself and writes the candidates in the order of the final records (tpos, chunk, ref, alt).  Else the
// capture's proposals counted them per tile, the scan places the tiles, k_mask_emit_cells writes them out and the sort
// puts them in that order.  Unless spec the host reads the count in between and sizes by it.
int call_candidates(himut_ctx* c, CallPlan* P, const Chunks& C) {
    hipStream_t st = c->stream;
    himut_ctx::Call& K = c->call;
    Scalars* sc = c->d_scalars.as<Scalars>();
    uint32_t *tilecnt = K.d_tilecnt.as<uint32_t>(), *tileoff = K.d_tileoff2.as<uint32_t>();
    const bool tiles = P->by_rank ? c->n > 0 : P->anyw > 0;      // (no reads: the front has built no column index)
    RankMask M;
    M.X = P->F.X; M.cells = K.d_mask.as<uint16_t>(); M.ncells = P->F.rmask_cells;
    M.cstart = c->d_cstart.as<int32_t>(); M.cend = c->d_cend.as<int32_t>(); M.nch = P->T.n;
    M.blkchunk = c->d_blkchunk.as<int32_t>(); M.nbc = c->n_blkchunk;
    uint32_t* tiletot = tileoff;                                 // by rank: the tiles' bits (there is no scan of them)
    if (tiles && P->by_rank) {
        hipLaunchKernelGGL(k_mask_count, dim3(P->mtiles), dim3(256), 0, st, M, P->F.idx_per, tiletot);
    } else if (tiles) {
        if (P->mtiles <= 65536u)
            hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(1024), 0, st, tilecnt, tileoff, (int)P->mtiles);
        else
            HCHECK(rocprim::exclusive_scan(c->d_tmp2.p, P->scan_tiles, tilecnt, tileoff, 0u, (size_t)P->mtiles, rocprim::plus<uint32_t>(), st));
    }
    if (!P->spec) {                                          // number of candidate evaluations -> record capacity
        uint32_t last_tcnt = 0, last_toff = 0;
        std::vector<uint32_t> tot(tiles && P->by_rank ? (size_t)P->mtiles : 0);      // (at most 1024 of them)
        if (!tot.empty()) {
            HCHECK(hipMemcpyAsync(tot.data(), tiletot, tot.size() * 4, hipMemcpyDeviceToHost, st));
        } else if (tiles) {
            HCHECK(hipMemcpyAsync(&last_tcnt, tilecnt + (P->mtiles - 1), 4, hipMemcpyDeviceToHost, st));
            HCHECK(hipMemcpyAsync(&last_toff, tileoff + (P->mtiles - 1), 4, hipMemcpyDeviceToHost, st));
        }
        HCHECK(hipMemcpyAsync(c->h_scalars, sc, sizeof(Scalars), hipMemcpyDeviceToHost, st));
        HCHECK(hipStreamSynchronize(st));
        if (const int err = reinterpret_cast<const Scalars*>(c->h_scalars)->err) return check_device_err(c, err);
        P->ncap = (int64_t)last_toff + last_tcnt;
        for (const uint32_t t : tot) P->ncap += t;
        P->nreserve = P->ncap + P->ncap / 4 + 1024;
        call_reserve_records(c, P);
    }
    if (P->ncap > 0 && P->by_rank) {
        hipLaunchKernelGGL(k_mask_emit, dim3(P->mtiles), dim3(256), 0, st, M, P->F.idx_per, tiletot, K.d_cands2.as<Cand>(),
                           K.d_keys2.as<uint64_t>(), P->ncap, &sc->ncand);
    } else if (P->ncap > 0) {
        hipLaunchKernelGGL(k_mask_emit_cells, dim3(P->mtiles), dim3(256), 0, st, K.d_posbits_c.as<uint32_t>(), (int64_t)P->T.positions,
                           K.d_mask.as<uint16_t>(), tileoff, C, K.d_cands.as<Cand>(), K.d_keys.as<uint64_t>(), P->ncap, &sc->ncand, tilecnt);
        HCHECK(rocprim::radix_sort_pairs(c->d_tmp.p, P->sort_tmp, K.d_keys.as<uint64_t>(), K.d_keys2.as<uint64_t>(), K.d_cands.as<uint64_t>(),
                                         K.d_cands2.as<uint64_t>(), (size_t)P->ncap, 0, 60, st));
    }
    stage_event(c, EV_EMIT, 2, st);
    return HIMUT_OK;
}

// .. EV_SWEEP: a thread per candidate column
void call_eval(himut_ctx* c, const CallPlan& P, const Reads& R, const Derived& D, const Chunks& C, const Phase& H) {
    Scalars* sc = c->d_scalars.as<Scalars>();
    if (P.ncap > 0) {
        EvalArgs A;
        A.P = c->params;
        A.S = site_sets(c);
        A.lut = c->d_lut.as<GtLut>();
        A.cands = c->call.d_cands2.as<Cand>(); A.ncand = P.ncap; A.ncand_dev = &sc->ncand;
        A.R = R; A.D = D; A.C = C; A.H = H; A.X = P.F.X;
        A.colstore = c->call.d_colstore.as<uint16_t>(); A.nslots = (int64_t)P.F.slot_cap;
        A.recs = c->call.d_recs.as<himut_record>();
        A.err = &sc->err;
        hipLaunchKernelGGL(P.phase ? k_eval_columns<true> : k_eval_columns<false>, dim3(blocks_for(P.ncap, 256)), dim3(256), 0, c->stream, A);
    }
    stage_event(c, EV_SWEEP, 2, c->stream);
}

// the finalisation: order, cross-chunk som_seen, counters, compaction (every set mask bit is one evaluation)
void call_finalize(himut_ctx* c, const CallPlan& P) {
    hipStream_t st = c->stream;
    himut_ctx::Call& K = c->call;
    Scalars* sc = c->d_scalars.as<Scalars>();
    if (P.ncap > 0) {
        const unsigned nb = blocks_for(P.ncap, 256);
        hipLaunchKernelGGL(k_finalize_flags, dim3(nb), dim3(256), 0, st, K.d_recs.as<himut_record>(), K.d_keys2.as<uint64_t>(),
                           &sc->ncand, P.ncap, K.d_emit.as<uint32_t>(), K.d_logpart.as<uint32_t>(),
                           c->d_ccs.as<uint8_t>(), c->n);
        hipLaunchKernelGGL(k_run_totals, dim3(1), dim3(1024), 0, st, P.ncap, K.d_blkoff.as<uint32_t>(), K.d_blkslots.as<uint32_t>(), P.F.X,
                           &sc->nrec, &sc->nslots, K.d_logpart.as<uint32_t>(), (int64_t)nb, sc->log, K.d_pos.as<uint32_t>());
        hipLaunchKernelGGL(k_compact, dim3(nb), dim3(256), 0, st, K.d_recs.as<himut_record>(), K.d_emit.as<uint32_t>(),
                           K.d_pos.as<uint32_t>(), &sc->ncand, P.ncap, K.d_recs_out.as<himut_record>());
    } else if (c->n > 0) {
        launch_count_flags(c, sc);                           // no mask sweep ran: count the flagged reads here
    }
}

int finish_run(himut_ctx* c, bool* overflow);

int do_run_once(himut_ctx* c, bool allow_spec, bool* overflow, bool defer) {
    *overflow = false;
    c->call.pending.active = false;
    if (int rc = check_scan_inputs(c)) return rc;
    begin_run(c, c->call.out);
    c->params.unique_qnames = c->unique_qnames ? 1 : 0;

    CallPlan P;
    if (int rc = call_plan(c, allow_spec, &P)) return rc;
    const Reads R = make_reads(c);
    const Derived D = make_derived(c);
    const Chunks C = make_chunks(c, P.T.n);
    const Phase H = make_phase(c);
    front_decode(c, P.F, c->params, P.clear_all);
    if (P.phase && P.T.npairs > 0) launch_read_hap(c, R, D, C, H, P.T, c->d_scalars.as<Scalars>());
    stage_event(c, EV_HAP, 2, c->stream);
    if (int rc = front_capture(c, &P.F, C, H, c->params, P.by_rank ? Proposals::by_rank : Proposals::by_cell)) return rc;
    if (int rc = call_candidates(c, &P, C)) return rc;
    call_eval(c, P, R, D, C, H);
    call_finalize(c, P);
    front_tail(c, P.F);
    // what the second half (finish_run) needs: himut_run_begin returns here, with everything queued
    c->call.pending.active = true;
    c->call.pending.plan = P;
    if (defer) return HIMUT_OK;
    return finish_run(c, overflow);
}

// The host's half behind a run's last copy: waits for it (not for the stream), checks the device's error word and the
// counts against the capacities, takes the counters and the stage times.
int finish_run(himut_ctx* c, bool* overflow) {
    *overflow = false;
    const PendingRun Q = c->call.pending;
    c->call.pending.active = false;
    if (!Q.active) return HIMUT_OK;
    HCHECK(hipSetDevice(c->device));
    if (int rc = front_tail_wait(c, Q.plan.F)) return rc;
    const Scalars& hs = *reinterpret_cast<const Scalars*>(c->h_scalars);
    const int64_t ncap = Q.plan.ncap, slot_cap = (int64_t)Q.plan.F.slot_cap;
    const int64_t ncand = ncap > 0 ? (int64_t)hs.ncand : 0;
    const int64_t nslots = ncap > 0 ? (int64_t)hs.nslots : slot_cap;
    if (ncand > ncap || nslots > slot_cap) {             // only a run on kept capacities can get here
        *overflow = true;                                // (mask cells past the capacity may still be set: not clean)
        return HIMUT_OK;
    }
    c->call.mask_clean = true;      // the emit ran over every cell that was set (or nothing was set)
    if (!Q.plan.spec && c->chunks_in_order) { c->call.cap_cand = Q.plan.nreserve; c->call.cap_slots = kept_slot_cap((size_t)slot_cap); }
    c->call.out.n = ncap > 0 ? (int64_t)hs.nrec : 0;
    take_log(c->call.out, hs.log);
    if (ncap <= 0) c->call.out.log[0] = (int64_t)hs.nccs;     // (else counter 0 came with the others, k_finalize_flags)
    static const StageSpan stages[] = {{&himut_run_stats::ms_parse, EV_START, EV_PARSE}, {&himut_run_stats::ms_hap, EV_PARSE, EV_HAP},
                                       {&himut_run_stats::ms_index, EV_HAP, EV_INDEX},   {&himut_run_stats::ms_emit, EV_GATHER, EV_EMIT},
                                       {&himut_run_stats::ms_eval, EV_EMIT, EV_SWEEP},   {&himut_run_stats::ms_finalize, EV_SWEEP, EV_FINAL}};
    front_stats(c, stages, sizeof(stages) / sizeof(stages[0]), Q.plan.T.positions, ncand, c->call.out.n, nslots);
    return HIMUT_OK;
}

void forget_capacities(himut_ctx* c) { c->call.cap_cand = c->call.cap_slots = 0; }

int do_run(himut_ctx* c) {
    return run_repeating(c, [&](bool kept, bool* overflow) { return do_run_once(c, kept, overflow, false); }, [&] { forget_capacities(c); });
}

// himut_run in two halves.  begin: everything queued; on kept capacities (any run but a context's first on its reads
// and chunks) without waiting for anything.  end: the wait, the checks, and the second pass with exact sizes if a count
// did not fit.  Between the two the context must not be touched.
int do_run_begin(himut_ctx* c) {
    bool overflow = false;
    int rc = do_run_once(c, true, &overflow, true);
    if (rc == HIMUT_OK && !c->call.pending.plan.spec && c->call.pending.active) {     // sized with the host in the loop: nothing left to overlap
        rc = finish_run(c, &overflow);
        c->call.pending.active = false;
    }
    return rc;
}
int do_run_end(himut_ctx* c) {
    if (!c->call.pending.active) return HIMUT_OK;
    // (the first pass is the one himut_run_begin queued: only its host half is left)
    return run_repeating(c, [&](bool kept, bool* overflow) { return kept ? finish_run(c, overflow) : do_run_once(c, false, overflow, false); },
                         [&] { forget_capacities(c); });
}

}  // namespace

extern "C" {

int himut_run(himut_ctx* c) {
    if (!c) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int { return do_run(c); });
}
int himut_run_begin(himut_ctx* c) {
    if (!c) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int { return do_run_begin(c); });
}
int himut_run_end(himut_ctx* c) {
    if (!c) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int { return do_run_end(c); });
}

int himut_get_records(himut_ctx* c, const himut_record** records, int64_t* n) {
    if (!c || !records || !n) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int { return get_run_out(c, c->call.out, c->call.d_recs_out, records, n, nullptr); });
}

int himut_get_log(himut_ctx* c, int64_t out[15]) {
    if (!c || !out) return HIMUT_ERR_ARG;
    std::copy(c->call.out.log, c->call.out.log + 15, out);
    return HIMUT_OK;
}

int himut_get_stats(himut_ctx* c, himut_run_stats* out) {
    if (!c || !out) return HIMUT_ERR_ARG;
    *out = c->stats;
    return HIMUT_OK;
}

int himut_records_device(himut_ctx* c, const void** dev_ptr, int64_t* n) {
    if (!c || !dev_ptr || !n) return HIMUT_ERR_ARG;
    *dev_ptr = c->call.d_recs_out.p;
    *n = c->call.out.n;
    return HIMUT_OK;
}

int himut_copy_records_to_device(himut_ctx* c, void* dst, int64_t capacity_records) {
    if (!c || (!dst && c->call.out.n)) return HIMUT_ERR_ARG;
    if (capacity_records < c->call.out.n) return fail(c, HIMUT_ERR_ARG, "destination too small");
    return guarded(c, [&]() -> int {
        HCHECK(hipSetDevice(c->device));
        if (c->call.out.n)
            HCHECK(hipMemcpyAsync(dst, c->call.d_recs_out.p, (size_t)c->call.out.n * sizeof(himut_record), hipMemcpyDeviceToDevice, c->stream));
        HCHECK(hipStreamSynchronize(c->stream));
        return HIMUT_OK;
    });
}

}  // extern "C"
