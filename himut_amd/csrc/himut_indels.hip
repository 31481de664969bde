// libhimut_hip.so: the indels run (himut_run_indels, himut_get_indels) over the kernels of himut_indels.h.  The cs decode
// in front of it is the read pass every pipeline starts with (run_parse_stage, himut_front.hip), under a parameter block
// whose gates are open, as the bqcal run's; there is no column front: the regions become a sorted table of the run's own
// (sorted_regions; the chunk tables of the call run stay as they are), the read windows are indexed again
// (launch_window_index), the events are a counted key list (count_keys, sort_with_tmp: himut_ctx.h, as the dbs run's
// proposals), and the repeat on kept capacities (run_repeating) and the result block (RunOut) are the ones the other
// record runs use.  Everything up to the ordered events is one front (indel_front_check, indel_front_run) on an event
// list of the caller's: the indelcal run (himut_indelcal.hip) starts from it too.
#include <hip/hip_runtime.h>

#include <string.h>  // rocprim's texture iterator needs the host memset declared first
#include <rocprim/rocprim.hpp>

#include "himut_ctx.h"
#include "himut_indels.h"

using namespace himut;

namespace {

// bits of the sort: the type and length, and the anchors of the span the reads cover
int key_bits(int64_t nblk) {
    int b = IND_KEY_SHIFT + WIN_SHIFT;
    while (b < 40 && ((int64_t)1 << (b - IND_KEY_SHIFT - WIN_SHIFT)) < nblk) b++;
    return b;
}

// rocPRIM's sort of the first n keys with the events' indices (d_keys -> d_keys2, 0.. -> d_vals); tmp null: the temporary size alone
hipError_t sort_events(himut_ctx* c, IndelEventList& I, void* tmp, size_t& bytes, int64_t n, int bits) {
    return rocprim::radix_sort_pairs(tmp, bytes, I.d_keys.as<uint64_t>(), I.d_keys2.as<uint64_t>(), rocprim::counting_iterator<uint32_t>(0),
                                     I.d_vals.as<uint32_t>(), (size_t)n, 0, bits, c->stream);
}

void reserve_for_events(himut_ctx* c, IndelEventList& I, int64_t cap, int bits, void (*reserve_more)(himut_ctx*, int64_t)) {
    I.d_keys.reserve((size_t)cap * 8 + 256);
    I.d_keys2.reserve((size_t)cap * 8 + 256);
    I.d_vals.reserve((size_t)cap * 4 + 256);
    I.d_ev.reserve((size_t)cap * sizeof(IndelEvent) + 256);
    I.d_ord.reserve((size_t)cap * sizeof(IndelEvent) + 256);
    if (reserve_more) reserve_more(c, cap);
    if (cap > 0) sort_with_tmp(I.d_sorttmp, false, [&](void* tmp, size_t& bytes) { return sort_events(c, I, tmp, bytes, cap, bits); });
}

// the indels run's own buffers of an event capacity: the records in their slots and at the front, the workgroups' counts
void reserve_records(himut_ctx* c, int64_t cap) {
    himut_ctx::Indels& I = c->indels;
    const unsigned nwg = blocks_for(cap, 256);
    I.d_recs.reserve(((size_t)nwg * 256 + 1) * sizeof(himut_indel_record));
    I.d_recs_out.reserve(((size_t)nwg * 256 + 1) * sizeof(himut_indel_record));
    I.d_wgcnt.reserve((size_t)nwg * 4 + 64);
}

void launch_events(himut_ctx* c, IndelArgs A, int64_t cap, const IndelSomatic* som) {
    HCHECK(hipMemsetAsync(A.sc, 0, IND_SC_WORDS * 8, c->stream));
    A.cap = cap;
    if (som) hipLaunchKernelGGL(k_indel_events<SomRules>, dim3(blocks_for(c->n, 16)), dim3(256), 0, c->stream, A, som->rules);
    else hipLaunchKernelGGL(k_indel_events<NoRules>, dim3(blocks_for(c->n, 16)), dim3(256), 0, c->stream, A, NoRules{});
}

// One pass.  kept: the event buffers keep the capacity of the previous indels run; *overflow is set if the events did not
// fit (the caller runs again with exact sizes).  The host waits once in the middle, for the number of events (the sort
// and the grids behind it take it).
int indels_once(himut_ctx* c, const himut_indel_params& p, bool allow_spec, bool* overflow) {
    *overflow = false;
    if (int rc = indel_front_check(c, p.max_len, "himut_run_indels")) return rc;
    himut_ctx::Indels& I = c->indels;
    begin_run(c, I.out);
    hipStream_t st = c->stream;
    IndelFront F;
    indel_front_run(c, I.ev, p, allow_spec, 0, reserve_records, &F);
    IndelArgs& A = F.A;
    if (I.have_errtab) { A.tab_hit = I.d_errtab.as<double>(); A.tab_err = A.tab_hit + RUN_CELLS; }
    if (!F.over && F.nev > 0) {
        const unsigned nwg = blocks_for(F.nev, 256);
        A.recs = I.d_recs.as<himut_indel_record>(); A.wgcnt = I.d_wgcnt.as<uint32_t>();
        hipLaunchKernelGGL(k_indel_eval, dim3(nwg), dim3(256), 0, st, A);
        stage_event(c, EV_SWEEP, 2, st);
        hipLaunchKernelGGL((k_compact_runs<himut_indel_record, SlotRuns<himut_indel_record>>), dim3(nwg), dim3(256), 0, st, I.d_wgcnt.as<uint32_t>(),
                           SlotRuns<himut_indel_record>{I.d_recs.as<himut_indel_record>()}, I.d_recs_out.as<himut_indel_record>(), F.words + IND_SC_NREC);
    } else {
        stage_event(c, EV_SWEEP, 2, st);
    }
    HCHECK(hipEventRecord(c->ev[EV_FINAL], st));
    struct { Scalars s; unsigned long long w[IND_SC_WORDS]; } h;
    HCHECK(hipMemcpyAsync(&h, F.sc, sizeof(h), hipMemcpyDeviceToHost, st));
    HCHECK(hipStreamSynchronize(st));
    if (h.s.err) return check_device_err(c, h.s.err);
    if (F.over) {
        *overflow = true;
        return HIMUT_OK;
    }
    if (!F.spec && c->n > 0) I.ev.cap_events = F.cap;
    I.out.n = (int64_t)h.w[IND_SC_NREC];
    take_log(I.out, h.w + IND_SC_LOG);
    I.out.log[IND_LOG_EVENTS] = F.nev;

    c->stats.ms_total = elapsed_ms(c, EV_START, EV_FINAL);
    if (c->timing >= 2) {
        c->stats.ms_parse = elapsed_ms(c, EV_START, EV_PARSE);
        c->stats.ms_emit = c->n > 0 ? elapsed_ms(c, EV_PARSE, EV_INDEX) : 0.0;      // the events (and the host's look at their number)
        c->stats.ms_index = elapsed_ms(c, EV_INDEX, EV_GATHER);                     // their sort and exact order
        c->stats.ms_eval = elapsed_ms(c, EV_GATHER, EV_SWEEP);
        c->stats.ms_finalize = elapsed_ms(c, EV_SWEEP, EV_FINAL);
    }
    c->stats.n_reads = c->n; c->stats.read_bases = c->read_bases; c->stats.positions = F.positions;
    c->stats.n_candidates = F.nev; c->stats.n_records = I.out.n;
    return HIMUT_OK;
}

}  // namespace

namespace himut {

int indel_front_check(himut_ctx* c, int32_t max_len, const char* who) {
    if (max_len < 1 || max_len > 64) return fail(c, HIMUT_ERR_ARG, std::string(who) + ": max_len must be 1..64");
    return check_run_inputs(c, NEED_READS | NEED_REGIONS | NEED_REFERENCE | NEED_SPANS);
}

void indel_front_run(himut_ctx* c, IndelEventList& I, const himut_indel_params& p, bool allow_spec, size_t own_words,
                     void (*reserve_more)(himut_ctx*, int64_t cap), IndelFront* F, const IndelSomatic* som) {
    hipStream_t st = c->stream;
    // the regions by start, with the running maximum of their ends (in_region)
    const int64_t nreg = (int64_t)c->cstart.size();
    std::vector<int32_t> sstart, spmax;
    sorted_regions(c->cstart, c->cend, &sstart, &spmax);
    int64_t positions = 0;
    for (int64_t k = 0; k < nreg; k++) positions += (int64_t)c->cend[(size_t)k] - c->cstart[(size_t)k] + 1;
    // every anchor lies under a read: the windows span the reads
    const int64_t nblk = ((int64_t)(c->h_prefmax.empty() ? 0 : c->h_prefmax.back()) >> WIN_SHIFT) + 2;
    const int bits = key_bits(nblk);

    // every buffer whose size the host knows, before anything is queued
    const bool spec = allow_spec && I.cap_events > 0 && c->n > 0;
    const size_t sc_bytes = sizeof(Scalars) + (IND_SC_WORDS + own_words) * 8;
    alloc_derived(c);
    I.d_sc.reserve(sc_bytes);
    // (the read windows are the context's, a function of the pushed reads alone: blocks written again hold what they held;
    //  a block that had to grow holds nothing the column front could still count on)
    const uint64_t win_was = c->d_winlo.gen + c->d_winhi.gen;
    c->d_winlo.reserve((size_t)nblk * 4 + 64);
    c->d_winhi.reserve((size_t)nblk * 4 + 64);
    if (win_was != c->d_winlo.gen + c->d_winhi.gen) c->win_nblk = 0;
    if (spec) reserve_for_events(c, I, I.cap_events, bits, reserve_more);
    upload(I.d_sstart, sstart, st);
    upload(I.d_spmax, spmax, st);
    Scalars* sc = I.d_sc.as<Scalars>();        // (not the context's: the runs over the column front keep theirs as they left them)
    unsigned long long* words = reinterpret_cast<unsigned long long*>(I.d_sc.as<uint8_t>() + sizeof(Scalars));

    HCHECK(hipEventRecord(c->ev[EV_START], st));
    HCHECK(hipMemsetAsync(sc, 0, sc_bytes, st));
    Params P = open_gate_params(c, p.min_mapq);
    if (som) P.p.min_sequence_identity = som->min_sequence_identity;       // RF_IDENT_OK under the run's own threshold
    IndelArgs A{};
    A.p = p; A.R = make_reads(c); A.D = make_derived(c);
    A.refseq = c->d_refseq.as<uint8_t>(); A.reflen = c->reflen;
    A.s_start = I.d_sstart.as<int32_t>(); A.s_pmaxend = I.d_spmax.as<int32_t>(); A.nregion = nreg;
    A.winlo = c->d_winlo.as<int32_t>(); A.winhi = c->d_winhi.as<int32_t>();
    A.sc = words; A.err = &sc->err;

    KeyCount K{0, 0, false};                             // the events: their number, the capacity they had, whether it held them
    if (c->n > 0) {
        run_parse_stage(c, A.R, A.D, sc, &P);
        launch_window_index(c, A.R, nblk, st);
        if (som) som->read_pass(c, A, *som);
        K = count_keys(c, spec, I.cap_events, words + IND_SC_NEV,
                       [&](int64_t cap) { A.keys = I.d_keys.as<uint64_t>(); A.ev = I.d_ev.as<IndelEvent>(); launch_events(c, A, cap, som); },
                       [&](int64_t cap) { reserve_for_events(c, I, cap, bits, reserve_more); });
        stage_event(c, EV_INDEX, 2, st);
        if (!K.over && K.n > 0) {
            const int64_t nev = K.n;
            sort_with_tmp(I.d_sorttmp, true, [&](void* tmp, size_t& bytes) { return sort_events(c, I, tmp, bytes, nev, bits); });
            A.keys2 = I.d_keys2.as<uint64_t>(); A.vals = I.d_vals.as<uint32_t>(); A.ord = I.d_ord.as<IndelEvent>(); A.nev = nev;
            hipLaunchKernelGGL(k_indel_order, dim3(blocks_for(nev, 256)), dim3(256), 0, st, A);
        }
    } else {
        stage_event(c, EV_PARSE, 2, st);
        stage_event(c, EV_INDEX, 2, st);
    }
    stage_event(c, EV_GATHER, 2, st);
    F->A = A; F->sc = sc; F->words = words;
    F->nev = K.n; F->cap = K.cap; F->nblk = nblk; F->nreg = nreg; F->positions = positions;
    F->spec = spec; F->over = K.over;
}

}  // namespace himut

extern "C" {

int himut_run_indels(himut_ctx* c, const himut_indel_params* p) {
    if (!c) return HIMUT_ERR_ARG;
    if (!p) return fail(c, HIMUT_ERR_ARG, "himut_run_indels: bad argument");
    return guarded(c, [&]() -> int {
        return run_repeating(c, [&](bool kept, bool* overflow) { return indels_once(c, *p, kept, overflow); },
                             [&] { c->indels.ev.cap_events = 0; });
    });
}

int himut_get_indels(himut_ctx* c, const himut_indel_record** records, int64_t* n, int64_t log[13]) {
    if (!c || !records || !n) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int { return get_run_out(c, c->indels.out, c->indels.d_recs_out, records, n, log); });
}

}  // extern "C"
