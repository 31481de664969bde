// libhimut_hip.so: the read pass every pipeline starts with (the kernels of himut_reads.h); the column front the call
// run and the germline run both go through, from the sizes to the copy-back and the stage times (front_plan,
// front_decode, front_capture, front_tail, front_tail_wait, front_stats); the call run (himut_run, himut_run_begin /
// _end) over the kernels of himut_kernels.h as a sequence of steps (call_plan, call_candidates, call_eval,
// call_finalize, finish_run), its records and counters; the dense pile of himut_pile_counts.
#include <hip/hip_runtime.h>

#include <string.h>  // rocprim's texture iterator needs the host memset declared first
#include <rocprim/rocprim.hpp>

#include "himut_ctx.h"
#include "himut_kernels.h"
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
            HCHECK(hipMemsetAsync(c->call.d_mask.p, 0, c->call.d_mask.cap, side));
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
int front_capture(himut_ctx* c, ColumnFront* F, const Chunks& C, const Phase& H, const Params& P, uint32_t* mask, uint32_t* tilecnt) {
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
    }
    CaptureArgs G;
    G.R = make_reads(c); G.D = make_derived(c); G.X = F->X; G.colstore = c->call.d_colstore.as<uint16_t>(); G.nslots = (int64_t)F->slot_cap;
    G.r_begin = 0; G.r_end = c->n; G.bqsum = c->d_bqsum.as<uint32_t>(); G.err = &sc->err;
    // the proposals of a read (read filters, trim / window filters -> mask) are the tail of its capture wave
    G.C = C; G.H = H; G.P = P; G.mask = mask; G.tilecnt = tilecnt;
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

namespace {

void launch_pile_dense(himut_ctx* c, const Chunks& C, const Reads& R, const Derived& D, const ChunkTables& T, int* err) {
    hipStream_t st = c->stream;
    c->call.d_tiles.reserve((size_t)T.n_tiles * sizeof(TileInfo) + 64);
    hipLaunchKernelGGL(k_tile_index<PD_TP>, dim3(blocks_for(T.n_tiles, 256)), dim3(256), 0, st, R, C,
                       c->d_tileoff.as<int64_t>(), T.n_tiles, c->call.d_tiles.as<TileInfo>());
    DenseArgs A;
    A.R = R; A.D = D; A.C = C; A.tiles = c->call.d_tiles.as<TileInfo>(); A.n_tiles = T.n_tiles;
    A.counts = c->call.d_dense_counts.as<uint32_t>(); A.bqsum = c->call.d_dense_bqsum.as<uint32_t>(); A.err = err;
    hipLaunchKernelGGL((k_pile_dense<PD_TP, PD_RB, PD_NT>), dim3((unsigned)T.n_tiles), dim3(PD_NT), 0, st, A);
}

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
    P->n4 = ((int64_t)P->T.positions * 2 + 15) / 16;
    P->mask_bytes = (size_t)P->n4 * 16;
    P->anyw = ((int64_t)P->T.positions + 31) / 32;
    P->mtiles = blocks_for(P->anyw, 256);
    const uint64_t mask_was = K.d_mask.gen;
    K.d_mask.reserve(P->mask_bytes + 64);
    // the emit sweep zeroes what the proposals set: a buffer that went through a whole run is clean
    const bool clear_mask = !K.mask_clean || mask_was != K.d_mask.gen;
    K.mask_clean = false;
    const uint64_t tcnt_was = K.d_tilecnt.gen;
    K.d_tilecnt.reserve((size_t)P->mtiles * 4 + 64);
    K.d_tileoff2.reserve((size_t)P->mtiles * 4 + 64);
    P->clear_all = clear_mask || tcnt_was != K.d_tilecnt.gen;
    if (P->phase && P->T.n > 65535) return fail(c, HIMUT_ERR_ARG, "--phase: more than 65,535 chunks in one contig (k_read_hap takes a chunk per grid row)");
    if (P->phase) c->d_hap.reserve((size_t)P->T.npairs + 64);
    P->F = front_plan(c, P->spec, K.cap_slots);
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

// .. EV_EMIT: the candidates = the set bits of the mask.  The capture's proposals counted them per tile: the scan
// places the tiles, k_mask_emit writes them out, in the order of the final records (tpos, chunk, ref, alt) when the
// chunks are in order, else the sort puts them so.  Unless spec the host reads the count in between and sizes by it.
int call_candidates(himut_ctx* c, CallPlan* P, const Chunks& C) {
    hipStream_t st = c->stream;
    himut_ctx::Call& K = c->call;
    Scalars* sc = c->d_scalars.as<Scalars>();
    uint32_t *tilecnt = K.d_tilecnt.as<uint32_t>(), *tileoff = K.d_tileoff2.as<uint32_t>();
    if (P->anyw > 0) {
        if (P->mtiles <= 65536u)
            hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(1024), 0, st, tilecnt, tileoff, (int)P->mtiles);
        else
            HCHECK(rocprim::exclusive_scan(c->d_tmp2.p, P->scan_tiles, tilecnt, tileoff, 0u, (size_t)P->mtiles, rocprim::plus<uint32_t>(), st));
    }
    if (!P->spec) {                                          // number of candidate evaluations -> record capacity
        uint32_t last_tcnt = 0, last_toff = 0;
        if (P->anyw > 0) {
            HCHECK(hipMemcpyAsync(&last_tcnt, tilecnt + (P->mtiles - 1), 4, hipMemcpyDeviceToHost, st));
            HCHECK(hipMemcpyAsync(&last_toff, tileoff + (P->mtiles - 1), 4, hipMemcpyDeviceToHost, st));
        }
        HCHECK(hipMemcpyAsync(c->h_scalars, sc, sizeof(Scalars), hipMemcpyDeviceToHost, st));
        HCHECK(hipStreamSynchronize(st));
        if (const int err = reinterpret_cast<const Scalars*>(c->h_scalars)->err) return check_device_err(c, err);
        P->ncap = (int64_t)last_toff + last_tcnt;
        P->nreserve = P->ncap + P->ncap / 4 + 1024;
        call_reserve_records(c, P);
    }
    if (P->ncap > 0) {
        const bool sorted = c->chunks_in_order;              // (else into the sort's input)
        hipLaunchKernelGGL(k_mask_emit, dim3(P->mtiles), dim3(256), 0, st, K.d_posbits_c.as<uint32_t>(), (int64_t)P->T.positions,
                           K.d_mask.as<uint16_t>(), tileoff, C, (sorted ? K.d_cands2 : K.d_cands).as<Cand>(),
                           (sorted ? K.d_keys2 : K.d_keys).as<uint64_t>(), P->ncap, &sc->ncand, tilecnt);
        if (!sorted)
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
    if (int rc = front_capture(c, &P.F, C, H, c->params, c->call.d_mask.as<uint32_t>(), c->call.d_tilecnt.as<uint32_t>())) return rc;
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
    c->call.mask_clean = true;      // the emit sweep ran over every cell that was set (or nothing was set)
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

int himut_pile_counts(himut_ctx* c, int32_t p0, int32_t p1, uint32_t* counts, uint32_t* bqsum) {
    if (!c || !counts || !bqsum || p1 <= p0) return fail(c, HIMUT_ERR_ARG, "bad pile range");
    if (!c->have_reads || !c->have_params || !c->have_lut) return fail(c, HIMUT_ERR_ARG, "context not initialised");
    return guarded(c, [&]() -> int {
        HCHECK(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        // one pseudo chunk (p0, p1): its tiles cover rpos p0-1 .. p1-1, the columns p0 .. p1-1 are complete
        std::vector<int32_t> cs{p0}, ce{p1};
        ChunkTables T = upload_chunks(c, cs, ce);
        alloc_derived(c);
        Reads R = make_reads(c);
        Derived D = make_derived(c);
        Chunks C = make_chunks(c, 1);
        Scalars* sc = borrow_scalars(c);
        HCHECK(hipMemsetAsync(sc, 0, sizeof(Scalars), st));
        if (c->n > 0) run_parse_stage(c, R, D, sc);
        c->call.d_dense_counts.reserve((size_t)T.positions * 6 * 4 + 64);
        c->call.d_dense_bqsum.reserve((size_t)T.positions * 4 * 4 + 64);
        HCHECK(hipMemsetAsync(c->call.d_dense_counts.p, 0, (size_t)T.positions * 24, st));
        HCHECK(hipMemsetAsync(c->call.d_dense_bqsum.p, 0, (size_t)T.positions * 16, st));
        if (c->n > 0) launch_pile_dense(c, C, R, D, T, &sc->err);
        const int64_t npos = (int64_t)p1 - p0;
        HCHECK(hipMemcpyAsync(counts, c->call.d_dense_counts.as<uint32_t>() + 6, (size_t)npos * 24, hipMemcpyDeviceToHost, st));
        HCHECK(hipMemcpyAsync(bqsum, c->call.d_dense_bqsum.as<uint32_t>() + 4, (size_t)npos * 16, hipMemcpyDeviceToHost, st));
        Scalars hs;
        HCHECK(hipMemcpyAsync(&hs, sc, sizeof(Scalars), hipMemcpyDeviceToHost, st));
        HCHECK(hipStreamSynchronize(st));
        if (hs.err) return check_device_err(c, hs.err);
        return HIMUT_OK;
    });
}

}  // extern "C"
