// libhimut_hip.so: the indelcal run (himut_run_indelcal, himut_get_indelcal) over the kernels of himut_indelcal.h, and the
// table the indels run may read (himut_set_indel_error_table).  The front -- the cs decode, the events, their sort and exact
// order -- is the indels run's (indel_front_run, himut_indels.hip) on an event list of this run's own; behind it the
// variant marks, the event pass and the span sweep over every 256-position block between the first and the last region.
// The repeat on kept capacities is run_repeating, as the indels run's.
#include <hip/hip_runtime.h>

#include "himut_ctx.h"
#include "himut_indelcal.h"

using namespace himut;

namespace {

int indelcal_once(himut_ctx* c, const himut_indelcal_params& p, bool allow_spec, bool* overflow) {
    *overflow = false;
    if (p.min_alt_count < 0) return fail(c, HIMUT_ERR_ARG, "himut_run_indelcal: min_alt_count must not be negative");
    if (p.vaf_permille < 0 || p.vaf_permille > 1000) return fail(c, HIMUT_ERR_ARG, "himut_run_indelcal: vaf_permille must be 0..1000");
    if (int rc = indel_front_check(c, p.max_len, "himut_run_indelcal")) return rc;
    himut_ctx::Indelcal& I = c->indelcal;
    HCHECK(hipSetDevice(c->device));
    memset(I.table, 0, sizeof(I.table));
    memset(I.log, 0, sizeof(I.log));
    memset(&c->stats, 0, sizeof(c->stats));
    hipStream_t st = c->stream;

    // the anchors a run can have: inside a region, with the run's first position inside the string
    int64_t lo = INT64_MAX, hi = -1;
    for (size_t k = 0; k < c->cstart.size(); k++) {
        lo = std::min<int64_t>(lo, c->cstart[k]);
        hi = std::max<int64_t>(hi, c->cend[k]);
    }
    lo = std::max<int64_t>(lo, 0);
    hi = std::min<int64_t>(hi, c->reflen - 2);
    // the bitmap spans the string and the read windows (an anchor lies under a read), before anything is queued
    const int64_t nblk_reads = ((int64_t)(c->h_prefmax.empty() ? 0 : c->h_prefmax.back()) >> WIN_SHIFT) + 2;
    const size_t bits_bytes = (size_t)((std::max<int64_t>(c->reflen, nblk_reads << WIN_SHIFT) + 31) / 32 + 2) * 4;
    I.d_bits.reserve(bits_bytes);
    const int64_t nb = lo <= hi ? (hi >> WIN_SHIFT) - (lo >> WIN_SHIFT) + 1 : 0;      // blocks of the sweep
    I.d_blkflag.reserve((size_t)nb + 64);

    himut_indel_params ip{};
    ip.min_mapq = p.min_mapq; ip.max_len = p.max_len; ip.min_alt_count = p.min_alt_count;
    IndelFront F;
    indel_front_run(c, I.ev, ip, allow_spec, IC_WORDS, nullptr, &F);
    IndelcalArgs C{};
    C.A = F.A; C.min_alt_count = p.min_alt_count; C.vaf_permille = p.vaf_permille; C.nblk = F.nblk;
    C.bits = I.d_bits.as<uint32_t>(); C.w = F.words + IND_SC_WORDS;
    if (!F.over) {
        HCHECK(hipMemsetAsync(I.d_bits.p, 0, bits_bytes, st));
        const unsigned nwg = blocks_for(F.nev, 256);
        if (F.nev > 0) hipLaunchKernelGGL(k_indelcal_mark, dim3(nwg), dim3(256), 0, st, C);
        stage_event(c, EV_HAP, 2, st);
        if (F.nev > 0) hipLaunchKernelGGL(k_indelcal_events, dim3(nwg), dim3(256), 0, st, C);
        stage_event(c, EV_SWEEP, 2, st);
        if (nb > 0) {
            C.blk0 = lo >> WIN_SHIFT; C.nb = nb;
            C.cell_budget = I.dbg_budget > 0 ? (uint64_t)I.dbg_budget : (1ull << 31);
            C.blkflag = I.d_blkflag.as<uint8_t>();
            hipLaunchKernelGGL(k_indelcal_blocks, dim3(blocks_for(nb, 256)), dim3(256), 0, st, C, nb);
            // a resident grid, eight workgroups per CU, strides over the blocks: its workgroups add to the table once each
            const unsigned resident = (unsigned)std::min<int64_t>(nb, I.dbg_wgs > 0 ? I.dbg_wgs : (int64_t)c->n_cus * 8);
            hipLaunchKernelGGL(k_indelcal_spans, dim3(resident), dim3(256), 0, st, C);
        }
    } else {
        stage_event(c, EV_HAP, 2, st);
        stage_event(c, EV_SWEEP, 2, st);
    }
    HCHECK(hipEventRecord(c->ev[EV_FINAL], st));
    struct { Scalars s; unsigned long long w[IND_SC_WORDS + IC_WORDS]; } h;
    HCHECK(hipMemcpyAsync(&h, F.sc, sizeof(h), hipMemcpyDeviceToHost, st));
    HCHECK(hipStreamSynchronize(st));
    if (h.s.err) return check_device_err(c, h.s.err);
    if (F.over) {
        *overflow = true;
        return HIMUT_OK;
    }
    if (!F.spec && c->n > 0) I.ev.cap_events = F.cap;
    const unsigned long long *tab = h.w + IND_SC_WORDS + IC_W_TABLE, *cnt = h.w + IND_SC_WORDS + IC_W_CNT;
    int64_t sum[IC_COLS] = {};
    for (int k = 0; k < IC_TABLE; k++) {
        I.table[k] = (int64_t)tab[k];
        sum[k % IC_COLS] += I.table[k];
    }
    int64_t counted = 0;
    for (int k = IC_COL_EVENTS; k < IC_COLS; k++) counted += sum[k];
    const int64_t log[14] = {F.nev, (int64_t)h.w[IND_SC_LOG + IND_LOG_EDGE], (int64_t)h.w[IND_SC_LOG + IND_LOG_LONG],
                             (int64_t)h.w[IND_SC_LOG + IND_LOG_NBASE], (int64_t)cnt[IC_CNT_ANCHORS], (int64_t)cnt[IC_CNT_VARIANT_ANCHORS],
                             (int64_t)cnt[IC_CNT_EV_VARIANT], (int64_t)cnt[IC_CNT_OFFRUN], (int64_t)cnt[IC_CNT_PARTIAL], counted,
                             sum[IC_COL_RUNS], sum[IC_COL_EXCLUDED], (int64_t)cnt[IC_CNT_RUNS_LONG], sum[IC_COL_SPANS]};
    memcpy(I.log, log, sizeof(log));

    c->stats.ms_total = elapsed_ms(c, EV_START, EV_FINAL);
    if (c->timing >= 2) {
        c->stats.ms_parse = elapsed_ms(c, EV_START, EV_PARSE);
        c->stats.ms_emit = c->n > 0 ? elapsed_ms(c, EV_PARSE, EV_INDEX) : 0.0;      // the events (and the host's look at their number)
        c->stats.ms_index = elapsed_ms(c, EV_INDEX, EV_GATHER);                     // their sort and exact order
        c->stats.ms_hap = elapsed_ms(c, EV_GATHER, EV_HAP);                         // the bitmap's clearing and the variant marks
        c->stats.ms_eval = elapsed_ms(c, EV_HAP, EV_SWEEP);                         // the event pass
        c->stats.ms_finalize = elapsed_ms(c, EV_SWEEP, EV_FINAL);                   // the span sweep
    }
    c->stats.n_reads = c->n; c->stats.read_bases = c->read_bases; c->stats.positions = F.positions;
    c->stats.n_candidates = F.nev;
    return HIMUT_OK;
}

}  // namespace

extern "C" {

int himut_run_indelcal(himut_ctx* c, const himut_indelcal_params* p) {
    if (!c) return HIMUT_ERR_ARG;
    if (!p) return fail(c, HIMUT_ERR_ARG, "himut_run_indelcal: bad argument");
    return guarded(c, [&]() -> int {
        return run_repeating(c, [&](bool kept, bool* overflow) { return indelcal_once(c, *p, kept, overflow); },
                             [&] { c->indelcal.ev.cap_events = 0; });
    });
}

int himut_get_indelcal(himut_ctx* c, int64_t table[1280], int64_t log[14]) {
    if (!c || !table) return HIMUT_ERR_ARG;
    memcpy(table, c->indelcal.table, sizeof(c->indelcal.table));
    if (log) memcpy(log, c->indelcal.log, sizeof(c->indelcal.log));
    return HIMUT_OK;
}

int himut_debug_indelcal(himut_ctx* c, int sweep_workgroups, int64_t cell_budget) {
    if (!c || sweep_workgroups < 0 || cell_budget < 0) return HIMUT_ERR_ARG;
    c->indelcal.dbg_wgs = sweep_workgroups;
    c->indelcal.dbg_budget = cell_budget;
    return HIMUT_OK;
}

int himut_set_indel_error_table(himut_ctx* c, const double* l_hit, const double* l_err, int64_t n) {
    if (!c) return HIMUT_ERR_ARG;
    if (n == 0) {
        c->indels.have_errtab = false;
        return HIMUT_OK;
    }
    if (n != RUN_CELLS || !l_hit || !l_err)
        return fail(c, HIMUT_ERR_ARG, "himut_set_indel_error_table: n must be " + std::to_string(RUN_CELLS) + " with both arrays, or 0 to clear");
    return guarded(c, [&]() -> int {
        HCHECK(hipSetDevice(c->device));
        himut_ctx::Indels& I = c->indels;
        I.have_errtab = false;
        I.d_errtab.reserve((size_t)2 * RUN_CELLS * sizeof(double));
        HCHECK(hipMemcpyAsync(I.d_errtab.p, l_hit, RUN_CELLS * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HCHECK(hipMemcpyAsync(I.d_errtab.as<double>() + RUN_CELLS, l_err, RUN_CELLS * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HCHECK(hipStreamSynchronize(c->stream));
        I.have_errtab = true;
        return HIMUT_OK;
    });
}

}  // extern "C"
