// libhimut_hip.so: the sindels run (himut_run_sindels, himut_get_sindels) over the kernels of himut_sindels.h.  The front
// -- the cs decode, the events, their sort and exact order -- is the indels run's (indel_front_run, himut_indels.hip) on an
// event list of this run's own, with the run's identity threshold in the decode's parameter block, the reads' verdicts
// (k_sindel_reads) queued behind the decode and the per-event rules in the event kernel (IndelSomatic).  Behind it one
// evaluation kernel and the shared compaction.  The repeat on kept capacities is run_repeating, as the indels run's.
#include <hip/hip_runtime.h>

#include "himut_ctx.h"
#include "himut_sindels.h"

using namespace himut;

namespace {

// the run's own buffers of an event capacity: the records in their slots and at the front, the workgroups' counts
void reserve_records(himut_ctx* c, int64_t cap) {
    himut_ctx::Sindels& I = c->sindels;
    const unsigned nwg = blocks_for(cap, 256);
    I.d_recs.reserve(((size_t)nwg * 256 + 1) * sizeof(himut_sindel_record));
    I.d_recs_out.reserve(((size_t)nwg * 256 + 1) * sizeof(himut_sindel_record));
    I.d_wgcnt.reserve((size_t)nwg * 4 + 64);
}

// the reads' verdicts, queued by the front between the decode and the events
void read_pass(himut_ctx* c, const IndelArgs& A, const IndelSomatic& som) {
    SindelReadArgs S{};
    S.R = A.R; S.meta = A.D.meta;
    S.min_mapq = A.p.min_mapq; S.min_qv = som.min_qv;
    S.qlen_lower_limit = som.qlen_lower_limit; S.qlen_upper_limit = som.qlen_upper_limit;
    S.verdict = c->sindels.d_verdict.as<uint8_t>();
    S.w = A.sc + IND_SC_WORDS; S.err = A.err;
    hipLaunchKernelGGL(k_sindel_reads, dim3(blocks_for(c->n, 4)), dim3(256), 0, c->stream, S);
    stage_event(c, EV_HAP, 2, c->stream);
}

int check_params(himut_ctx* c, const himut_sindel_params& p) {
    if (!(p.min_trim >= 0.0 && p.min_trim <= 0.5)) return fail(c, HIMUT_ERR_ARG, "himut_run_sindels: min_trim must lie in [0, 0.5]");
    if (p.max_run < 0) return fail(c, HIMUT_ERR_ARG, "himut_run_sindels: max_run must not be negative");
    if (p.mismatch_window_size < 0) return fail(c, HIMUT_ERR_ARG, "himut_run_sindels: mismatch_window_size must not be negative");
    if (p.max_mismatch_count < 0) return fail(c, HIMUT_ERR_ARG, "himut_run_sindels: max_mismatch_count must not be negative");
    return indel_front_check(c, p.max_len, "himut_run_sindels");
}

int sindels_once(himut_ctx* c, const himut_sindel_params& p, bool allow_spec, bool* overflow) {
    *overflow = false;
    if (int rc = check_params(c, p)) return rc;
    himut_ctx::Sindels& I = c->sindels;
    begin_run(c, I.out);
    hipStream_t st = c->stream;
    I.d_verdict.reserve((size_t)c->n + 256);

    himut_indel_params ip{};
    ip.min_mapq = p.min_mapq; ip.min_gq = p.min_gq; ip.min_ref_count = p.min_ref_count; ip.min_alt_count = p.min_alt_count;
    ip.md_threshold = p.md_threshold; ip.max_len = p.max_len;
    ip.l_hit = p.l_hit; ip.l_err = p.l_err; ip.l_half = p.l_half;
    for (int g = 0; g < 3; g++) ip.prior[g] = p.prior[g];
    IndelSomatic som{};
    som.min_sequence_identity = p.min_sequence_identity;
    som.rules.verdict = I.d_verdict.as<uint8_t>();
    som.rules.min_bq = p.min_bq; som.rules.max_mismatch_count = p.max_mismatch_count;
    som.rules.mismatch_window_size = p.mismatch_window_size; som.rules.min_trim = p.min_trim;
    som.min_qv = p.min_qv; som.qlen_lower_limit = p.qlen_lower_limit; som.qlen_upper_limit = p.qlen_upper_limit;
    som.read_pass = read_pass;

    IndelFront F;
    indel_front_run(c, I.ev, ip, allow_spec, SIN_WORDS, reserve_records, &F, &som);
    SindelEvalArgs C{};
    C.A = F.A; C.max_run = p.max_run; C.w = F.words + IND_SC_WORDS;
    if (c->indels.have_errtab) { C.A.tab_hit = c->indels.d_errtab.as<double>(); C.A.tab_err = C.A.tab_hit + RUN_CELLS; }
    if (!F.over && F.nev > 0) {
        const unsigned nwg = blocks_for(F.nev, 256);
        C.recs = I.d_recs.as<himut_sindel_record>(); C.A.wgcnt = I.d_wgcnt.as<uint32_t>();
        hipLaunchKernelGGL(k_sindel_eval, dim3(nwg), dim3(256), 0, st, C);
        stage_event(c, EV_SWEEP, 2, st);
        hipLaunchKernelGGL((k_compact_runs<himut_sindel_record, SlotRuns<himut_sindel_record>>), dim3(nwg), dim3(256), 0, st, I.d_wgcnt.as<uint32_t>(),
                           SlotRuns<himut_sindel_record>{I.d_recs.as<himut_sindel_record>()}, I.d_recs_out.as<himut_sindel_record>(), F.words + IND_SC_NREC);
    } else {
        stage_event(c, EV_SWEEP, 2, st);
    }
    HCHECK(hipEventRecord(c->ev[EV_FINAL], st));
    struct { Scalars s; unsigned long long w[IND_SC_WORDS + SIN_WORDS]; } h;
    HCHECK(hipMemcpyAsync(&h, F.sc, sizeof(h), hipMemcpyDeviceToHost, st));
    HCHECK(hipStreamSynchronize(st));
    if (h.s.err) return check_device_err(c, h.s.err);
    if (F.over) {
        *overflow = true;
        return HIMUT_OK;
    }
    if (!F.spec && c->n > 0) I.ev.cap_events = F.cap;
    I.out.n = (int64_t)h.w[IND_SC_NREC];
    const unsigned long long *ind = h.w + IND_SC_LOG, *evr = h.w + IND_SC_SOM, *own = h.w + IND_SC_WORDS, *ev = own + SIN_W_EVAL;
    const int64_t log[SIN_NLOG] = {F.nev, (int64_t)ind[IND_LOG_EDGE], (int64_t)ind[IND_LOG_LONG], (int64_t)ind[IND_LOG_NBASE],
                                   (int64_t)own[SIN_W_PILE], (int64_t)own[SIN_W_PROPOSING], (int64_t)evr[IND_SOM_EVENTS], (int64_t)evr[IND_SOM_TRIM],
                                   (int64_t)evr[IND_SOM_WINDOW], (int64_t)evr[IND_SOM_LOWBQ], (int64_t)evr[IND_SOM_PROPOSING], (int64_t)ev[SIN_EV_CAND],
                                   (int64_t)ev[SIN_EV_GERM_HET], (int64_t)ev[SIN_EV_GERM_HOMALT], (int64_t)ev[SIN_EV_INDELSITE], (int64_t)ev[SIN_EV_REPEAT],
                                   (int64_t)ev[SIN_EV_LOWGQ], (int64_t)ev[SIN_EV_LOWDEPTH], (int64_t)ev[SIN_EV_HIGHDEPTH], (int64_t)ev[SIN_EV_PASS]};
    take_log(I.out, log);

    c->stats.ms_total = elapsed_ms(c, EV_START, EV_FINAL);
    if (c->timing >= 2) {
        c->stats.ms_parse = elapsed_ms(c, EV_START, EV_PARSE);
        c->stats.ms_hap = c->n > 0 ? elapsed_ms(c, EV_PARSE, EV_HAP) : 0.0;         // the window index and the reads' verdicts (every quality once)
        c->stats.ms_emit = c->n > 0 ? elapsed_ms(c, EV_HAP, EV_INDEX) : 0.0;        // the events (and the host's look at their number)
        c->stats.ms_index = elapsed_ms(c, EV_INDEX, EV_GATHER);                     // their sort and exact order
        c->stats.ms_eval = elapsed_ms(c, EV_GATHER, EV_SWEEP);
        c->stats.ms_finalize = elapsed_ms(c, EV_SWEEP, EV_FINAL);
    }
    c->stats.n_reads = c->n; c->stats.read_bases = c->read_bases; c->stats.positions = F.positions;
    c->stats.n_candidates = F.nev; c->stats.n_records = I.out.n;
    return HIMUT_OK;
}

}  // namespace

extern "C" {

int himut_run_sindels(himut_ctx* c, const himut_sindel_params* p) {
    if (!c) return HIMUT_ERR_ARG;
    if (!p) return fail(c, HIMUT_ERR_ARG, "himut_run_sindels: bad argument");
    return guarded(c, [&]() -> int {
        return run_repeating(c, [&](bool kept, bool* overflow) { return sindels_once(c, *p, kept, overflow); },
                             [&] { c->sindels.ev.cap_events = 0; });
    });
}

int himut_get_sindels(himut_ctx* c, const himut_sindel_record** records, int64_t* n, int64_t log[20]) {
    if (!c || !records || !n) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int { return get_run_out(c, c->sindels.out, c->sindels.d_recs_out, records, n, log); });
}

}  // extern "C"
