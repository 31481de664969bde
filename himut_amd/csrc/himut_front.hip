// libhimut_hip.so: the read pass every pipeline starts with (the kernels of himut_reads.h) and the column front the
// call, germline, dbs and sites runs go through (the kernels of himut_front.h), from the sizes to the copy-back and the
// stage times (front_plan, front_decode, front_capture, front_totals, front_tail, front_tail_wait, front_stats); the
// read pass's debug exports.  The only unit that compiles those two headers' kernels.
#include <hip/hip_runtime.h>

#include <string.h>  // rocprim's texture iterator needs the host memset declared first
#include <rocprim/rocprim.hpp>

#include "himut_ctx.h"
#include "himut_front.h"
#include "himut_reads.h"

using namespace himut;

namespace himut {

// ---- the read pass

namespace {

// What the decode does beside decoding.  P: the parameter block its gate reads (null: the call run's, himut_set_params).
// bits, nwords: the bitmap of column positions the gate sets (null: none).  fill: the column store, to be left EMPTY
// (fill_slots 16-bit slots) by the decode's waves.
struct ParseSide {
    const Params* P = nullptr;
    uint32_t* bits = nullptr;
    int64_t nwords = 0;
    void* fill = nullptr;
    int64_t fill_slots = 0;
};

// The group plan of the pushed reads (k_group_flags, himut_reads.h): which reads start a group, compacted into the
// groups' first reads.  A function of cs_off alone, made once per batch like the window index: by the first decode
// behind himut_push_reads or an ingest, which waits here for the number of groups (the grid of every decode of the
// batch); forget_reads drops it.
void ensure_group_plan(himut_ctx* c) {
    if (c->plan_valid) return;
    hipStream_t st = c->stream;
    const int64_t n = c->n;
    c->d_gflag.reserve((size_t)n + 64);
    c->d_gfirst.reserve((size_t)(n + 1) * 4 + 64);
    c->d_gcount.reserve(64);
    size_t tmp = 0;
    HCHECK(rocprim::select(nullptr, tmp, rocprim::counting_iterator<int32_t>(0), c->d_gflag.as<uint8_t>(), c->d_gfirst.as<int32_t>(),
                           c->d_gcount.as<unsigned long long>(), (size_t)n, st));
    c->d_gtmp.reserve(tmp + 256);
    const bool timed = c->dbg_decode_on;          // (tests) plan_ms: between two of the context's events, free at this point
    if (timed) HCHECK(hipEventRecord(c->ev[EV_SIDE], st));
    hipLaunchKernelGGL(k_group_flags, dim3(blocks_for(n, 256)), dim3(256), 0, st, n, c->d_csoff.as<int64_t>(), c->dbg_decode == 1 ? 1 : 0,
                       c->d_gflag.as<uint8_t>());
    HCHECK(rocprim::select(c->d_gtmp.p, tmp, rocprim::counting_iterator<int32_t>(0), c->d_gflag.as<uint8_t>(), c->d_gfirst.as<int32_t>(),
                           c->d_gcount.as<unsigned long long>(), (size_t)n, st));
    if (timed) HCHECK(hipEventRecord(c->ev[EV_HAP], st));
    unsigned long long ng = 0;
    HCHECK(hipMemcpyAsync(&ng, c->d_gcount.p, 8, hipMemcpyDeviceToHost, st));
    HCHECK(hipStreamSynchronize(st));
    c->plan_ms = timed ? elapsed_ms(c, EV_SIDE, EV_HAP) : 0.0;
    c->n_groups = (int64_t)ng;
    c->plan_valid = true;
}

// the cs decode on c->stream: a wave per group of the plan
void launch_parse(himut_ctx* c, const Reads& R, const Derived& D, Scalars* sc, const ParseSide& S) {
    ensure_group_plan(c);
    const int64_t ng = c->n_groups;
    const int64_t fill16 = (S.fill_slots * 2 + 15) / 16;
    const int fill_per = S.fill ? (int)((fill16 + ng * 64 - 1) / (ng * 64)) : 0;
    unsigned long long* dbg = nullptr;
    if (c->dbg_decode_on) {                       // (tests) the decode's counters, and behind it a copy of the bitmap it set
        c->d_dbgcnt.reserve(64);
        if (S.bits) c->d_dbgbits.reserve((size_t)S.nwords * 4 + 64);
        dbg = c->d_dbgcnt.as<unsigned long long>();
        HCHECK(hipMemsetAsync(dbg, 0, 32, c->stream));
    }
    hipLaunchKernelGGL(k_parse_cs, dim3(blocks_for(ng, 4)), dim3(256), 0, c->stream, R, D, S.P ? *S.P : c->params, &sc->err,
                       c->d_ccs.as<uint8_t>(), S.bits, S.nwords, (uint4*)S.fill, fill16, fill_per, c->d_gfirst.as<int32_t>(), ng, c->any_longcs ? 1 : 0, dbg);
    if (c->dbg_decode_on) {
        c->dbg_bits_words = S.bits ? S.nwords : 0;
        if (S.bits) HCHECK(hipMemcpyAsync(c->d_dbgbits.p, S.bits, (size_t)S.nwords * 4, hipMemcpyDeviceToDevice, c->stream));
    }
}

void check_longcs(himut_ctx* c, const Reads& R, const Derived& D, Scalars* sc) {
    if (c->any_longcs)
        hipLaunchKernelGGL(k_check_longcs, dim3(blocks_for(c->n, 256)), dim3(256), 0, c->stream, R, D, &sc->err);
}

// The decode with work beside it: begin launches the decode and returns the side stream, which starts behind EV_START
// (the previous run on this context is over by then) and takes the caller's work that needs nothing from the decode;
// join brings it back in front of whatever follows the decode on c->stream.
hipStream_t parse_stage_begin(himut_ctx* c, const Reads& R, const Derived& D, Scalars* sc, const ParseSide& S) {
    launch_parse(c, R, D, sc, S);
    HCHECK(hipStreamWaitEvent(c->side, c->ev[EV_START], 0));
    return c->side;
}

void parse_stage_join(himut_ctx* c, const Reads& R, const Derived& D, Scalars* sc) {
    HCHECK(hipEventRecord(c->ev[EV_SIDE], c->side));
    check_longcs(c, R, D, sc);
    HCHECK(hipStreamWaitEvent(c->stream, c->ev[EV_SIDE], 0));
    stage_event(c, EV_PARSE, 2, c->stream);
}

}  // namespace

void run_parse_stage(himut_ctx* c, const Reads& R, const Derived& D, Scalars* sc, const Params* P) {
    parse_stage_begin(c, R, D, sc, ParseSide{P});
    parse_stage_join(c, R, D, sc);
}

void flag_bases_once(himut_ctx* c, hipStream_t st) {
    if (c->bases_flagged) return;             // (d_nonacgt is sized by alloc_derived)
    if (c->n > 0)
        hipLaunchKernelGGL(k_flag_bases, dim3(blocks_for(c->n, 4)), dim3(256), 0, st, c->n, c->d_qoff.as<int64_t>(), c->d_qlen.as<int32_t>(),
                           c->d_seq.as<uint8_t>(), c->d_nonacgt.as<uint8_t>());
    c->bases_flagged = true;
}

void launch_window_index(himut_ctx* c, const Reads& R, int64_t nblk, hipStream_t st) {
    hipLaunchKernelGGL(k_window_index, dim3(blocks_for(nblk, 256)), dim3(256), 0, st, R, nblk, c->d_winlo.as<int32_t>(),
                       c->d_winhi.as<int32_t>());
}

void launch_read_hap(himut_ctx* c, const Reads& R, const Derived& D, const Chunks& C, const Phase& H, const ChunkTables& T, Scalars* sc) {
    hipLaunchKernelGGL(k_read_hap, dim3((unsigned)blocks_for(T.maxpairs, 16), (unsigned)T.n), dim3(256), 0, c->stream, R, D, C, H, &sc->err);
}

void launch_count_flags(himut_ctx* c, Scalars* sc) {
    hipLaunchKernelGGL(k_count_flags, dim3(256), dim3(256), 0, c->stream, c->d_ccs.as<uint8_t>(), c->n, &sc->nccs);
}

void alloc_derived(himut_ctx* c) {
    const int64_t n = c->n;
    const int64_t segcap = (c->cs_bytes >> 1) + n + 2;
    c->d_bqsum.reserve((size_t)n * 4 + 64);
    c->d_nseg.reserve((size_t)n * 4 + 64);
    c->d_nmis.reserve((size_t)n * 4 + 64);
    c->d_nnsub.reserve((size_t)n * 4 + 64);
    c->d_segs.reserve((size_t)segcap * sizeof(Seg));
    c->d_mis.reserve((size_t)segcap * 4);
    c->d_mq.reserve((size_t)segcap * 4);
    c->d_meta.reserve((size_t)(n + 1) * sizeof(ReadMeta));
    c->d_rflag.reserve((size_t)n + 64);
    c->d_ccs.reserve((size_t)n + 64);
    c->d_scalars.reserve(sizeof(Scalars));
    c->d_nonacgt.reserve((size_t)n + 64);
}

// ---- the column front (himut_ctx.h): one implementation for the call run and the germline run

ColumnFront front_plan(himut_ctx* c, bool spec, int64_t kept_slots, bool span_chunks) {
    ColumnFront F;
    // bitmap of column positions: probed at every position a read covers, so it spans reads as well as chunks; the
    // read windows and the column offsets are kept per 256 positions of the same span
    int32_t maxpos = c->h_prefmax.empty() ? 0 : c->h_prefmax.back();
    if (span_chunks)
        for (int32_t e : c->cend) maxpos = std::max(maxpos, e);
    F.nblk = ((int64_t)maxpos >> WIN_SHIFT) + 2;
    F.nwords = F.nblk * 8;
    F.lead_bytes = (size_t)(F.nwords + 2) * 4;
    // the column index: a thread per `idx_per` consecutive blocks, at most 1024 workgroups (k_block_sums / k_block_table3)
    F.idx_per = (int)std::max<int64_t>(1, (F.nblk + 256 * 1024 - 1) / (256 * 1024));
    F.idx_wgs = blocks_for(F.nblk, 256 * F.idx_per);
    F.spec = spec;
    F.slot_cap = spec ? (size_t)kept_slots : 0;
    // sized before anything is queued: growing a buffer in the middle of a run would free it under the kernels already
    // queued on it
    c->d_winlo.reserve((size_t)F.nblk * 4 + 64);
    c->d_winhi.reserve((size_t)F.nblk * 4 + 64);
    const uint64_t bits_was = c->call.d_posbits_c.gen;
    c->call.d_posbits_c.reserve(F.lead_bytes + 256);
    if (bits_was != c->call.d_posbits_c.gen) c->lead_clean_bytes = 0;      // another block, whatever its address: not the one left empty
    c->call.d_posrank.reserve((size_t)F.idx_wgs * sizeof(uint4) + 256);      // per-workgroup totals of the column index
    c->call.d_blkslots.reserve((size_t)F.nblk * 4 + 256); c->call.d_blkoff.reserve((size_t)F.nblk * 4 + 256);
    c->call.d_blktab.reserve((size_t)F.nblk * sizeof(BlockTab) + 256);
    // (on kept capacities the column store's size is known before the decode has run: the decode's waves fill it)
    if (spec) c->call.d_colstore.reserve(F.slot_cap * 2 + 256);
    F.X.bits = c->call.d_posbits_c.as<uint32_t>(); F.X.rank = nullptr; F.X.nwords = F.nwords;
    F.X.bt = c->call.d_blktab.as<BlockTab>(); F.X.nblk = F.nblk;
    return F;
}

void front_decode(himut_ctx* c, const ColumnFront& F, const Params& P, bool clear_mask) {
    hipStream_t st = c->stream;
    const Reads R = make_reads(c);
    const Derived D = make_derived(c);
    Scalars* sc = c->d_scalars.as<Scalars>();
    uint32_t* bits = c->call.d_posbits_c.as<uint32_t>();
    HCHECK(hipEventRecord(c->ev[EV_START], st));
    flag_bases_once(c, st);
    // The cs decode sets the bits of the column positions and every kernel adds to the scalars: both are empty before
    // the run starts.  A run leaves them so (it clears them behind its last copy, while the host is already reading
    // the results): only a context that has not just been through a run over this front pays for the fills here.
    if (c->lead_clean_bytes < F.lead_bytes) {
        HCHECK(hipMemsetAsync(sc, 0, sizeof(Scalars), st));
        HCHECK(hipMemsetAsync(bits, 0, F.lead_bytes, st));
    }
    c->lead_clean_bytes = 0;
    // The read windows per 256 positions depend on the pushed reads only (like a BAM index they are made once per
    // batch: the first run after himut_push_reads).  That kernel and the fills of a mask that is not known to be
    // empty need nothing from the cs decode: they run beside it on the second stream.  A context that has been
    // through a run has neither to do, and the second stream stays idle.
    const bool need_win = c->n > 0 && c->win_nblk != F.nblk;
    auto side_work = [&](hipStream_t side) {
        if (clear_mask) {
            if (c->call.d_mask.p) HCHECK(hipMemsetAsync(c->call.d_mask.p, 0, c->call.d_mask.cap, side));
            HCHECK(hipMemsetAsync(c->call.d_tilecnt.p, 0, c->call.d_tilecnt.cap, side));
        }
        if (need_win) launch_window_index(c, R, F.nblk, side);
    };
    if (c->n <= 0) {
        side_work(st);
        stage_event(c, EV_PARSE, 2, st);
        return;
    }
    // (a null fill: the decode does not look at the slot count)
    const ParseSide S{&P, bits, F.nwords, F.spec ? c->call.d_colstore.p : nullptr, (int64_t)F.slot_cap};
    if (clear_mask || need_win) {
        side_work(parse_stage_begin(c, R, D, sc, S));
        parse_stage_join(c, R, D, sc);
    } else {
        launch_parse(c, R, D, sc, S);
        check_longcs(c, R, D, sc);
        stage_event(c, EV_PARSE, 2, st);
    }
    c->win_nblk = F.nblk;
}

// columns: per 256-position block the column positions and the read window -> one scan -> the block table -> the capture
int front_capture(himut_ctx* c, ColumnFront* F, const Chunks& C, const Phase& H, const Params& P, Proposals proposals) {
    hipStream_t st = c->stream;
    if (c->n <= 0) {
        F->slot_cap = 0; F->marked = 0;
        stage_event(c, EV_INDEX, 1, st);
        stage_event(c, EV_GATHER, 1, st);
        return HIMUT_OK;
    }
    Scalars* sc = c->d_scalars.as<Scalars>();
    const int64_t nblk = F->nblk;
    BlockCount BC;
    BC.bits = c->call.d_posbits_c.as<uint32_t>(); BC.winlo = c->d_winlo.as<int32_t>(); BC.winhi = c->d_winhi.as<int32_t>();
    hipLaunchKernelGGL(k_block_sums, dim3(F->idx_wgs), dim3(256), 0, st, BC, nblk, F->idx_per, c->call.d_posrank.as<uint4>());
    hipLaunchKernelGGL(k_block_table3, dim3(F->idx_wgs), dim3(256), 0, st, BC, nblk, F->idx_per, c->call.d_posrank.as<uint4>(),
                       c->call.d_blktab.as<BlockTab>(), c->call.d_blkoff.as<uint32_t>(), c->call.d_blkslots.as<uint32_t>(), &sc->err);
    if (!F->spec) {
        Scalars& hs = *reinterpret_cast<Scalars*>(c->h_scalars);
        uint32_t last_off = 0, last_n = 0;
        BlockTab last{};
        HCHECK(hipMemcpyAsync(&last_off, c->call.d_blkoff.as<uint32_t>() + (nblk - 1), 4, hipMemcpyDeviceToHost, st));
        HCHECK(hipMemcpyAsync(&last_n, c->call.d_blkslots.as<uint32_t>() + (nblk - 1), 4, hipMemcpyDeviceToHost, st));
        HCHECK(hipMemcpyAsync(&last, c->call.d_blktab.as<BlockTab>() + (nblk - 1), sizeof(BlockTab), hipMemcpyDeviceToHost, st));
        HCHECK(hipMemcpyAsync(&hs, sc, sizeof(Scalars), hipMemcpyDeviceToHost, st));
        HCHECK(hipStreamSynchronize(st));
        if (hs.err) return check_device_err(c, hs.err);
        const size_t slot_cap = (size_t)last_off + last_n;
        F->slot_cap = slot_cap;
        F->marked = (int64_t)last.ufirst + (int64_t)(last.ncnt >> 22);      // (front_totals_of, himut_emit.h, from the host's three words)
        c->call.d_colstore.reserve((size_t)kept_slot_cap(slot_cap) * 2 + 256);
        if (slot_cap) HCHECK(hipMemsetD16Async(c->call.d_colstore.p, (unsigned short)CELL_EMPTY, slot_cap, st));
        if (proposals == Proposals::by_rank) {
            // the mask by rank has a cell per marked position and chunk: sized like the column store, with its headroom.
            // A block that is new holds anything; one that was there has been cleared beside the decode if it had to be
            DevBuf& M = c->call.d_mask;
            const uint64_t mask_was = M.gen;
            M.reserve(rank_mask_bytes((size_t)kept_slot_cap(slot_cap), C.n));
            if (mask_was != M.gen) HCHECK(hipMemsetAsync(M.p, 0, M.cap, st));
            F->rmask_cells = kept_slot_cap(slot_cap) + C.n;
        }
    }
    CaptureArgs G;
    G.R = make_reads(c); G.D = make_derived(c); G.X = F->X; G.colstore = c->call.d_colstore.as<uint16_t>(); G.nslots = (int64_t)F->slot_cap;
    G.r_begin = 0; G.r_end = c->n; G.bqsum = c->d_bqsum.as<uint32_t>(); G.err = &sc->err;
    // the proposals of a read (read filters, trim / window filters -> mask) are the tail of its capture wave
    if (proposals == Proposals::by_rank && F->rmask_cells <= 0) return fail(c, HIMUT_ERR_ARG, "the mask by rank has no size");
    const bool prop = proposals != Proposals::none;
    G.C = C; G.H = H; G.P = P; G.mask = prop ? c->call.d_mask.as<uint32_t>() : nullptr; G.tilecnt = prop ? c->call.d_tilecnt.as<uint32_t>() : nullptr;
    G.rcells = proposals == Proposals::by_rank ? F->rmask_cells : 0;
    G.ccs_flag = c->d_ccs.as<uint8_t>();
    stage_event(c, EV_INDEX, 1, st);
    hipLaunchKernelGGL(k_stream_capture, dim3(blocks_for(c->n, 4)), dim3(256), 0, st, G);
    stage_event(c, EV_GATHER, 1, st);
    return HIMUT_OK;
}

void front_totals(himut_ctx* c, const ColumnFront& F, unsigned long long* sc, int i_marked, int i_slots) {
    hipLaunchKernelGGL(k_front_totals, dim3(1), dim3(64), 0, c->stream, F.X, c->call.d_blkoff.as<uint32_t>(), c->call.d_blkslots.as<uint32_t>(), sc,
                       i_marked, i_slots);
}

void front_tail(himut_ctx* c, const ColumnFront& F) {
    hipStream_t st = c->stream;
    Scalars* sc = c->d_scalars.as<Scalars>();
    HCHECK(hipEventRecord(c->ev[EV_FINAL], st));
    HCHECK(hipMemcpyAsync(c->h_scalars, sc, sizeof(Scalars), hipMemcpyDeviceToHost, st));
    HCHECK(hipEventRecord(c->ev[EV_COPIED], st));
    HCHECK(hipMemsetAsync(sc, 0, sizeof(Scalars), st));
    HCHECK(hipMemsetAsync(c->call.d_posbits_c.p, 0, F.lead_bytes, st));
}

int front_tail_wait(himut_ctx* c, const ColumnFront& F) {
    HCHECK(hipEventSynchronize(c->ev[EV_COPIED]));
    if (const int err = reinterpret_cast<const Scalars*>(c->h_scalars)->err) return check_device_err(c, err);
    c->lead_clean_bytes = F.lead_bytes;
    return HIMUT_OK;
}

void front_stats(himut_ctx* c, const StageSpan* stages, size_t n_stages, int64_t positions, int64_t n_candidates, int64_t n_records,
                 int64_t column_slots) {
    himut_run_stats& S = c->stats;
    S.ms_total = elapsed_ms(c, EV_START, EV_FINAL);
    if (c->timing >= 1) S.ms_capture = elapsed_ms(c, EV_INDEX, EV_GATHER);
    for (size_t k = 0; k < n_stages && c->timing >= 2; k++) S.*stages[k].ms = elapsed_ms(c, stages[k].from, stages[k].to);
    S.n_reads = c->n; S.read_bases = c->read_bases; S.positions = positions;
    S.n_candidates = n_candidates; S.n_records = n_records; S.column_slots = column_slots;
}

}  // namespace himut

extern "C" {

int himut_debug_decode(himut_ctx* c, int mode) {
    if (!c || mode < 0 || mode > 1) return fail(c, HIMUT_ERR_ARG, "bad decode mode");
    c->dbg_decode = mode;
    c->dbg_decode_on = true;
    c->plan_valid = false;
    return HIMUT_OK;
}

int himut_debug_read_pass_sizes(himut_ctx* c, int64_t* out) {
    if (!c || !out) return HIMUT_ERR_ARG;
    out[0] = c->n;
    out[1] = c->n > 0 ? (c->cs_bytes >> 1) + c->n + 2 : 0;
    out[2] = c->dbg_bits_words;
    return HIMUT_OK;
}

int himut_debug_read_pass(himut_ctx* c, int32_t* nseg, int32_t* nmis, int32_t* nnsub, uint8_t* rflag, void* meta, void* segs, int32_t* mis,
                          uint32_t* mq, uint32_t* bits, int64_t* counters, double* plan_ms) {
    if (!c || !nseg || !nmis || !nnsub || !rflag || !meta || !segs || !mis || !mq || !counters || !plan_ms) return HIMUT_ERR_ARG;
    if (!c->dbg_decode_on || !c->plan_valid) return fail(c, HIMUT_ERR_ARG, "no read pass under himut_debug_decode yet");
    return guarded(c, [&]() -> int {
        HCHECK(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        const size_t n = (size_t)c->n, slots = (size_t)((c->cs_bytes >> 1) + c->n + 2);
        if (n) {
            HCHECK(hipMemcpyAsync(nseg, c->d_nseg.p, n * 4, hipMemcpyDeviceToHost, st));
            HCHECK(hipMemcpyAsync(nmis, c->d_nmis.p, n * 4, hipMemcpyDeviceToHost, st));
            HCHECK(hipMemcpyAsync(nnsub, c->d_nnsub.p, n * 4, hipMemcpyDeviceToHost, st));
            HCHECK(hipMemcpyAsync(rflag, c->d_rflag.p, n, hipMemcpyDeviceToHost, st));
            HCHECK(hipMemcpyAsync(meta, c->d_meta.p, n * sizeof(ReadMeta), hipMemcpyDeviceToHost, st));
            HCHECK(hipMemcpyAsync(segs, c->d_segs.p, slots * sizeof(Seg), hipMemcpyDeviceToHost, st));
            HCHECK(hipMemcpyAsync(mis, c->d_mis.p, slots * 4, hipMemcpyDeviceToHost, st));
            HCHECK(hipMemcpyAsync(mq, c->d_mq.p, slots * 4, hipMemcpyDeviceToHost, st));
        }
        if (bits && c->dbg_bits_words) HCHECK(hipMemcpyAsync(bits, c->d_dbgbits.p, (size_t)c->dbg_bits_words * 4, hipMemcpyDeviceToHost, st));
        unsigned long long cnt[4] = {0, 0, 0, 0};
        if (c->d_dbgcnt.p) HCHECK(hipMemcpyAsync(cnt, c->d_dbgcnt.p, 32, hipMemcpyDeviceToHost, st));
        HCHECK(hipStreamSynchronize(st));
        for (int i = 0; i < 4; i++) counters[i] = (int64_t)cnt[i];
        *plan_ms = c->plan_ms;
        return HIMUT_OK;
    });
}

}  // extern "C"
