// libhimut_hip.so: normcounts (himut_run_normcounts) over the kernels of himut_norm.h and himut_normq.h, and the
// resident reference string it sweeps (himut_set_reference).
#include <hip/hip_runtime.h>

#include "himut_ctx.h"
#include "himut_normq.h"

using namespace himut;

namespace {

// A contig takes up to three passes (do_normcounts), each a whole one, read pass included.  First: k_norm_quad (a wave
// per 256 columns), k_norm_dirty for the positions it lists, k_norm_tile for the tiles it lists.  MoreRoom: the same
// after a First pass whose list of positions was too short in some part (a region where more than one position in four
// holds another allele: deep piles, a sample far from the reference), with the room that pass's counters ask for -- the
// context keeps it, as a density, for its later passes, as himut_run keeps its capacities.  Tile: the whole contig with
// k_norm_tile, when the list of tiles was too short (or the room still is, which the counters rule out).
// (NormPass and NormPlan: himut_ctx.h, with the front's steps the callable run takes too.)
enum class NormOutcome { Done, NeedsRoom, NeedsTile };

NormOutcome norm_outcome(NormPass pass, bool dirty_over, unsigned nredo, unsigned redo_cap) {
    if (pass == NormPass::Tile || !(dirty_over || nredo > redo_cap)) return NormOutcome::Done;
    if (pass == NormPass::First && nredo <= redo_cap) return NormOutcome::NeedsRoom;
    return NormOutcome::NeedsTile;
}

// entries of a part of the position list whose workgroup sweeps n positions: room for a quarter of them and some slack
// (a column with another allele is one in thirty), never for more than all of them; after a pass that ran out, for the
// density that pass needed (dirty_room: entries per NQ_WG_COLS positions)
int64_t part_cap(const himut_ctx* c, int64_t n) {
    int64_t cap = n / 4 + std::min<int64_t>(64, n / 4 + 8);
    if (c->norm.dirty_room > 0) cap = std::max(cap, (n * c->norm.dirty_room + NQ_WG_COLS - 1) / NQ_WG_COLS + 8);
    return std::min(cap, n);
}

}  // namespace

namespace himut {

// The sweep's scratch, laid out by each chunk's own length (phase blocks range from one position to megabases): tile k
// of chunk j is row toff[j] + k of the plan, and workgroup x of chunk j lists the positions it leaves to k_norm_dirty
// in entries [doff[q_gx j + x], doff[q_gx j + x + 1]) of one list, part_cap of them unless a test caps the parts
// (dbg_cap > 0).  The table is built and uploaded again only when the chunks, the room or the test's cap changed: a
// contig's passes over the same chunks reuse it.  Fills n_tiles and n_dirty.
void norm_layout(himut_ctx* c, NormPlan* P, int64_t dbg_cap) {
    himut_ctx::Norm& N = c->norm;
    const int64_t n_ch = P->T.n, q_gx = P->q_gx, G = q_gx / 8;
    std::vector<int64_t>& lay = N.h_lay;
    if (!(N.lay_ok && N.lay_room == N.dirty_room && N.lay_dbg == dbg_cap && N.lay_cs == c->cstart && N.lay_ce == c->cend)) {
        lay.assign((size_t)(n_ch + 1 + P->q_regions + 1), 0);
        N.h_swept.assign((size_t)P->q_regions, 0);                                      // positions per workgroup
        int64_t* toff = lay.data();
        int64_t* doff = toff + n_ch + 1;
        for (int64_t k = 0; k < n_ch; k++) {
            const int64_t len = std::max<int64_t>((int64_t)c->cend[k] - c->cstart[k], 0);
            toff[k + 1] = toff[k] + (len + NQ_COLS - 1) / NQ_COLS;
            const int64_t per = std::min<int64_t>(P->q_per, ((len + NQ_WG_COLS - 1) / NQ_WG_COLS + 7) / 8);   // (k_norm_quad's mapping)
            for (int64_t x = 0; x < q_gx; x++) {
                int64_t n = 0;
                for (int64_t t = x >> 3; t < per; t += G)
                    n += std::min<int64_t>(std::max<int64_t>(len - ((x & 7) * per + t) * NQ_WG_COLS, 0), NQ_WG_COLS);
                N.h_swept[(size_t)(k * q_gx + x)] = n;
            }
        }
        for (int64_t r = 0; r < P->q_regions; r++) {
            const int64_t cap = part_cap(c, N.h_swept[(size_t)r]);
            doff[r + 1] = doff[r] + (dbg_cap > 0 ? std::min(cap, dbg_cap) : cap);
        }
        upload(N.d_lay, lay.data(), lay.size(), c->stream);
        N.lay_ok = true; N.lay_room = N.dirty_room; N.lay_dbg = dbg_cap;
        N.lay_cs = c->cstart; N.lay_ce = c->cend;
    }
    P->n_tiles = lay[(size_t)n_ch];
    P->n_dirty = lay[(size_t)(n_ch + 1 + P->q_regions)];
    P->d_toff = N.d_lay.as<int64_t>();
    P->d_doff = P->d_toff + n_ch + 1;
}

// The sizes of a pass, all in one place (a kernel that leaves its buffers ends the process, not the call), and EVERY
// buffer of the pass reserved for them before anything of the pass is queued: DevBuf::reserve drains the device when
// it grows, and growing a buffer in the middle of a pass would free it under the kernels already queued on it.  Nothing
// behind EV_START reserves.
NormPlan norm_plan(himut_ctx* c, const ChunkTables& T, NormPass pass) {
    NormPlan P;
    himut_ctx::Norm& N = c->norm;
    P.T = T;
    P.phase = c->params.p.phase != 0;
    P.work = c->n > 0 && T.n > 0;
    P.quad = pass != NormPass::Tile && N.dbg_sweep != 1;                                // (1: a test asks for k_norm_tile)
    P.ntri = (size_t)c->ref_K * c->ref_K * c->ref_K;
    // the sweep's grid (workgroups of NQ_WAVES waves, a wave per 256 positions; NQ_Q workgroups per XCD class and chunk)
    int32_t maxend = 0;
    for (size_t k = 0; k < c->cstart.size(); k++) {
        P.maxspan = std::max(P.maxspan, c->cend[k] - c->cstart[k]);
        maxend = std::max(maxend, c->cend[k]);
    }
    const int64_t n1 = std::max<int64_t>(T.n, 1);
    P.q_per = ((int64_t)blocks_for(P.maxspan, NQ_WG_COLS) + 7) / 8;
    // (NQ_Q workgroups per class and chunk keep a wave on a dozen tiles of a long contig; a contig of a few chunks gets
    //  more of them, so that the grid still fills the chip: about 4096 workgroups where the tiles allow)
    const int64_t q_want = std::max<int64_t>(NQ_Q, (4096 + 8 * n1 - 1) / (8 * n1));
    P.q_gx = 8u * (unsigned)std::min<int64_t>(q_want, P.q_per);
    P.q_regions = (int64_t)P.q_gx * n1;
    P.nblk = ((int64_t)maxend >> WIN_SHIFT) + 2;
    // the read pass's buffers, then the sweep's scratch (in the order a context has always allocated them)
    alloc_derived(c);
    if (P.phase) c->d_hap.reserve((size_t)T.npairs + 64);
    N.d_tri.reserve((2 * P.ntri + 16) * 8);
    N.d_live.reserve((size_t)c->n + 64);
    N.d_callable.reserve(((size_t)(c->bq_bytes >> 5) + 64) * 4);
    norm_layout(c, &P, pass == NormPass::First ? N.dbg_dirty_cap : 0);                  // (tests: the first pass overflows)
    // tiles left to k_norm_tile (more pieces than the plan holds, more columns with another allele than a wave's pool): room for
    // every tile of the contig
    P.redo_cap = (unsigned)std::min<int64_t>(P.n_tiles + 64, (int64_t)1 << 28);
    if (P.quad) {
        N.d_dirty.reserve((size_t)P.n_dirty * sizeof(NormDirty) + 256);
        N.d_dcount.reserve((size_t)P.q_regions * 4 + 256);
        N.d_redo.reserve((size_t)P.redo_cap * sizeof(NormRedo) + 256);
    }
    c->d_winlo.reserve((size_t)P.nblk * 4 + 64);
    c->d_winhi.reserve((size_t)P.nblk * 4 + 64);
    if (P.quad && P.work) {                                                             // k_norm_plan's rows
        N.d_plan.reserve((size_t)P.n_tiles * NQ_ITEMS * sizeof(NqItem) + 256);
        N.d_plancnt.reserve((size_t)P.n_tiles * 4 + 256);
    }
    P.R = make_reads(c); P.D = make_derived(c); P.C = make_chunks(c, T.n); P.H = make_phase(c);
    P.sc = borrow_scalars(c);
    return P;
}

// EV_START .. EV_EMIT: the decode, the read filters, the callable bits, the reads' haplotypes, the window index
void norm_read_pass(himut_ctx* c, const NormPlan& P) {
    hipStream_t st = c->stream;
    uint8_t* live = c->norm.d_live.as<uint8_t>();
    uint8_t* ccs = c->d_ccs.as<uint8_t>();
    HCHECK(hipEventRecord(c->ev[EV_START], st));
    flag_bases_once(c, st);
    HCHECK(hipMemsetAsync(P.sc, 0, sizeof(Scalars), st));
    HCHECK(hipMemsetAsync(ccs, 0, (size_t)c->n + 1, st));
    HCHECK(hipMemsetAsync(c->norm.d_tri.p, 0, (2 * P.ntri + 16) * 8, st));
    // (d_callable is not cleared: k_callable writes the words of every read)
    if (c->n > 0) run_parse_stage(c, P.R, P.D, P.sc);   // (the quality sums are k_callable's)
    else stage_event(c, EV_PARSE, 2, st);
    if (P.work) {
        hipLaunchKernelGGL(k_read_live, dim3(blocks_for(c->n, 16)), dim3(256), 0, st, P.R, P.D, P.C, c->params, live, ccs, &P.sc->err);
        // (k_callable takes the reads with a low mean quality out of `live`: before the phased runs' count of the reads)
        hipLaunchKernelGGL(k_callable, dim3(blocks_for(c->n, 4)), dim3(256), 0, st, P.R, P.D, c->params, live,
                           c->norm.d_callable.as<uint32_t>(), ccs);
        if (P.phase && P.T.npairs > 0) {
            launch_read_hap(c, P.R, P.D, P.C, P.H, P.T, P.sc);
            hipLaunchKernelGGL(k_pair_ccs, dim3(blocks_for(P.T.npairs, 256)), dim3(256), 0, st, P.C, P.H, P.R, live, P.T.npairs, ccs);
        }
        launch_window_index(c, P.R, P.nblk, st);
    }
    HCHECK(hipEventRecord(c->ev[EV_EMIT], st));
}

NormArgs norm_args(himut_ctx* c, const NormPlan& P, const uint8_t* alt_order, int non_human) {
    NormArgs A{};
    A.P = c->params;
    A.S = site_sets(c);
    A.lut = c->d_lut.as<GtLut>();
    A.R = P.R; A.C = P.C; A.H = P.H;
    A.refseq = c->d_refseq.as<uint8_t>(); A.reflen = c->reflen;
    memcpy(A.cls, c->ref_cls, 256);
    A.K = c->ref_K; A.cA = c->ref_cls['A']; A.cC = c->ref_cls['C']; A.cG = c->ref_cls['G']; A.cT = c->ref_cls['T'];
    memcpy(A.alt_order, alt_order, 12);
    A.non_human = non_human;
    A.ccs_tri = c->norm.d_tri.as<unsigned long long>(); A.ref_tri = A.ccs_tri + P.ntri; A.log = A.ccs_tri + 2 * P.ntri;
    A.err = &P.sc->err;
    return A;
}

}  // namespace himut

namespace {

// the plan: which pieces of which reads lie over each tile of 256 positions (k_norm_plan); the sweep (k_norm_quad);
// the positions and the tiles it listed (k_norm_dirty, k_norm_tile)
void norm_sweep_quad(himut_ctx* c, const NormPlan& P, const NormArgs& A) {
    hipStream_t st = c->stream;
    himut_ctx::Norm& N = c->norm;
    const int32_t* winlo = c->d_winlo.as<int32_t>();
    const int32_t* winhi = c->d_winhi.as<int32_t>();
    const uint32_t* callable = N.d_callable.as<uint32_t>();
    NormRedo* redo = N.d_redo.as<NormRedo>();
    const int64_t tpc = (int64_t)blocks_for(P.maxspan, NQ_COLS);                        // tiles of the longest chunk (the grid)
    const dim3 pgrid((unsigned)blocks_for(blocks_for(tpc, NQ_PLAN_TILES), 4), (unsigned)P.T.n);
    hipLaunchKernelGGL(P.phase ? k_norm_plan<true> : k_norm_plan<false>, pgrid, dim3(256), 0, st, A, P.D, winlo, winhi, P.nblk, P.d_toff,
                       N.d_plan.as<NqItem>(), N.d_plancnt.as<uint32_t>(), redo, &P.sc->nredo, P.redo_cap);
    stage_event(c, EV_INDEX, 1, st);                                                    // (around k_norm_quad: stats.ms_capture)
    const unsigned pool_limit = N.dbg_pool > 0 ? (unsigned)std::min(N.dbg_pool, NQ_SLOTS) : (unsigned)NQ_SLOTS;
    hipLaunchKernelGGL(P.phase ? k_norm_quad<true> : k_norm_quad<false>, dim3(P.q_gx, (unsigned)P.T.n), dim3(NQ_WAVES * 64), 0, st, A,
                       callable, (int64_t)c->bq_bytes, N.d_refcode.as<uint16_t>(), N.d_plan.as<NqItem>(), N.d_plancnt.as<uint32_t>(),
                       P.d_toff, P.q_per, N.d_dirty.as<NormDirty>(), P.d_doff, N.d_dcount.as<uint32_t>(), &P.sc->dirty_over, redo,
                       &P.sc->nredo, P.redo_cap, pool_limit);
    stage_event(c, EV_GATHER, 1, st);
    hipLaunchKernelGGL(k_norm_dirty, dim3((unsigned)std::min<int64_t>(blocks_for(P.q_regions, 4), 16384)), dim3(256), 0, st, A,
                       N.d_dirty.as<NormDirty>(), N.d_dcount.as<uint32_t>(), P.d_doff, P.q_regions);
    // (returns at once unless a tile was listed)
    hipLaunchKernelGGL(k_norm_tile, dim3(1024), dim3(256), 0, st, A, P.D, callable, winlo, winhi, P.nblk, (int64_t)0, redo,
                       &P.sc->nredo, P.redo_cap);
}

// the whole contig with k_norm_tile: the tiles of a chunk dealt to the XCD classes, NT_Q workgroups per class and chunk
void norm_sweep_tile(himut_ctx* c, const NormPlan& P, const NormArgs& A) {
    const int64_t per = ((int64_t)blocks_for(P.maxspan, 256) + 7) / 8;
    const dim3 grid(8u * (unsigned)std::min<int64_t>(NT_Q, per), (unsigned)P.T.n);
    hipLaunchKernelGGL(k_norm_tile, grid, dim3(256), 0, c->stream, A, P.D, c->norm.d_callable.as<uint32_t>(), c->d_winlo.as<int32_t>(),
                       c->d_winhi.as<int32_t>(), P.nblk, per, (const NormRedo*)nullptr, (const unsigned int*)nullptr, 0u);
}

// The host's tail behind EV_FINAL: the histograms and the scalars back, what the pass came to (for a pass that is to
// be repeated nothing else is looked at: the device's error word after the decision), the counters and the stage times.
int norm_finish(himut_ctx* c, const NormPlan& P, NormPass pass, NormOutcome* outcome) {
    hipStream_t st = c->stream;
    std::vector<unsigned long long>& h_tri = c->norm.h_tri;
    h_tri.assign(2 * P.ntri + 16, 0ULL);
    Scalars hs;
    HCHECK(hipMemcpyAsync(h_tri.data(), c->norm.d_tri.p, (2 * P.ntri + 16) * 8, hipMemcpyDeviceToHost, st));
    HCHECK(hipMemcpyAsync(&hs, P.sc, sizeof(Scalars), hipMemcpyDeviceToHost, st));
    HCHECK(hipStreamSynchronize(st));
    // (tests, sweep = 2: the first pass as if the list of tiles had been too short)
    const unsigned nredo = pass == NormPass::First && c->norm.dbg_sweep == 2 ? P.redo_cap + 1 : hs.nredo;
    *outcome = norm_outcome(pass, hs.dirty_over != 0, nredo, P.redo_cap);
    if (*outcome == NormOutcome::NeedsRoom) {            // the largest density a part's counter asks for, an eighth on top
        std::vector<uint32_t> need((size_t)P.q_regions);
        HCHECK(hipMemcpy(need.data(), c->norm.d_dcount.p, (size_t)P.q_regions * 4, hipMemcpyDeviceToHost));
        int64_t room = c->norm.dirty_room;
        for (int64_t r = 0; r < P.q_regions; r++) {
            const int64_t v = need[(size_t)r], n = c->norm.h_swept[(size_t)r];   // (under the test's cap alone: nothing raised)
            if (n > 0 && v > part_cap(c, n)) room = std::max(room, ((v + v / 8) * NQ_WG_COLS + n - 1) / n);
        }
        c->norm.dirty_room = room;
    }
    if (*outcome != NormOutcome::Done) return HIMUT_OK;
    himut_run_stats& S = c->stats;
    S.reran = pass != NormPass::First ? 1 : 0;
    if (hs.err) return check_device_err(c, hs.err);
    h_tri[2 * P.ntri + 0] = hs.nccs;
    S.ms_total = elapsed_ms(c, EV_START, EV_FINAL);
    if (c->timing >= 2) {   // recorded by run_parse_stage only then (an unrecorded event leaves a sticky HIP error)
        S.ms_parse = elapsed_ms(c, EV_START, EV_PARSE);
        S.ms_index = elapsed_ms(c, EV_PARSE, EV_EMIT);              // the read pass: filters, callable bits, window index
    }
    S.ms_eval = elapsed_ms(c, EV_EMIT, EV_FINAL);                   // the position sweep: plan, k_norm_quad, k_norm_dirty, listed tiles
    if (c->timing >= 1 && P.quad && P.work)
        S.ms_capture = elapsed_ms(c, EV_INDEX, EV_GATHER);          // k_norm_quad by itself, the pass's dominant kernel
    S.n_reads = c->n; S.read_bases = c->read_bases; S.positions = P.T.positions;
    S.column_slots = hs.nredo;               // (normcounts: tiles k_norm_quad left to k_norm_tile)
    c->norm.have = true;
    c->norm.cal_words = P.work ? (c->bq_bytes >> 5) : 0;
    c->norm.cal_reads = P.work ? c->n : 0;
    return HIMUT_OK;
}

int do_normcounts(himut_ctx* c, const uint8_t* alt_order, int non_human) {
    if (int rc = check_scan_inputs(c, true)) return rc;
    for (int k = 0; k < 12; k++) if (alt_order[k] > 3) return fail(c, HIMUT_ERR_ARG, "alt_order holds alleles 0..3");
    HCHECK(hipSetDevice(c->device));
    c->norm.have = false;
    memset(&c->stats, 0, sizeof(c->stats));
    c->params.unique_qnames = c->unique_qnames ? 1 : 0;
    if (c->cstart.size() > 65535) return fail(c, HIMUT_ERR_ARG, "more than 65,535 chunks in one contig (the sweep's grids take a chunk per row)");
    NormPass pass = NormPass::First;
    for (int k = 0; k < 3; k++) {                        // (First, MoreRoom, Tile at the most: a Tile pass is always done)
        const NormPlan P = norm_plan(c, upload_chunks(c, c->cstart, c->cend), pass);
        norm_read_pass(c, P);
        if (P.work) {
            const NormArgs A = norm_args(c, P, alt_order, non_human);
            if (P.quad) norm_sweep_quad(c, P, A);
            else norm_sweep_tile(c, P, A);
            launch_count_flags(c, P.sc);
        }
        HCHECK(hipEventRecord(c->ev[EV_FINAL], c->stream));
        NormOutcome outcome = NormOutcome::Done;
        if (int rc = norm_finish(c, P, pass, &outcome)) return rc;
        if (outcome == NormOutcome::Done) return HIMUT_OK;
        pass = outcome == NormOutcome::NeedsRoom ? NormPass::MoreRoom : NormPass::Tile;
    }
    return fail(c, HIMUT_ERR_ARG, "normcounts: the whole-contig sweep asked for another pass");
}

}  // namespace

extern "C" {

int himut_set_reference(himut_ctx* c, const uint8_t* seq, int64_t len, const uint8_t* cls, int n_classes) {
    if (!c) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int {
        if (!seq || len <= 0 || !cls || n_classes < 5 || n_classes > 32) return fail(c, HIMUT_ERR_ARG, "bad reference / class table");
        HCHECK(hipSetDevice(c->device));
        c->strands.n = 0;             // the segment list (himut_set_strands) was the old string's
        upload(c->d_refseq, seq, (size_t)len, c->stream);
        // the letters' codes for the sweep, with room behind the string (a tile's last lanes read past it: codes of 0)
        c->norm.d_refcode.reserve(((size_t)len + 512) * 2);
        hipLaunchKernelGGL(k_ref_codes, dim3(2048), dim3(256), 0, c->stream, c->d_refseq.as<uint8_t>(), len, c->norm.d_refcode.as<uint16_t>(), len + 512);
        HCHECK(hipStreamSynchronize(c->stream));
        c->reflen = len;
        memcpy(c->ref_cls, cls, 256);
        c->ref_K = n_classes;
        for (int k = 0; k < 256; k++) if (cls[k] >= n_classes) return fail(c, HIMUT_ERR_ARG, "class id out of range");
        return HIMUT_OK;
    });
}

int himut_run_normcounts(himut_ctx* c, const uint8_t* alt_order, int non_human_sample) {
    if (!c || !alt_order) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int { return do_normcounts(c, alt_order, non_human_sample); });
}

int himut_debug_normcounts(himut_ctx* c, int sweep, int64_t dirty_cap, int pool_slots) {
    if (!c || sweep < 0 || sweep > 2 || dirty_cap < 0 || pool_slots < 0) return HIMUT_ERR_ARG;
    c->norm.dbg_sweep = sweep; c->norm.dbg_dirty_cap = dirty_cap; c->norm.dbg_pool = pool_slots;
    return HIMUT_OK;
}

int himut_debug_norm_scratch(himut_ctx* c, int64_t out[4]) {
    if (!c || !out) return HIMUT_ERR_ARG;
    out[0] = (int64_t)(c->norm.d_plan.cap + c->norm.d_plancnt.cap);
    out[1] = (int64_t)(c->norm.d_dirty.cap + c->norm.d_dcount.cap + c->norm.d_lay.cap);
    out[2] = (int64_t)c->norm.d_redo.cap;
    out[3] = out[0] + out[1] + out[2];
    return HIMUT_OK;
}

int himut_debug_norm_callable(himut_ctx* c, uint32_t* words, int64_t n_words, uint8_t* live, int64_t n_reads) {
    if (!c) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int {
        if (!c->norm.have) return fail(c, HIMUT_ERR_ARG, "himut_run_normcounts has not completed");
        if (n_words < 0 || n_reads < 0 || (n_words > 0 && !words) || (n_reads > 0 && !live))
            return fail(c, HIMUT_ERR_ARG, "himut_debug_norm_callable: bad arguments");
        if (n_words > c->norm.cal_words || n_reads > c->norm.cal_reads)
            return fail(c, HIMUT_ERR_ARG, "himut_debug_norm_callable: more words or reads than the pass wrote");
        HCHECK(hipSetDevice(c->device));
        HCHECK(hipStreamSynchronize(c->stream));
        if (n_words > 0) HCHECK(hipMemcpy(words, c->norm.d_callable.p, (size_t)n_words * 4, hipMemcpyDeviceToHost));
        if (n_reads > 0) HCHECK(hipMemcpy(live, c->norm.d_live.p, (size_t)n_reads, hipMemcpyDeviceToHost));
        return HIMUT_OK;
    });
}

int himut_get_normcounts(himut_ctx* c, int64_t* ccs_tri, int64_t* ref_tri, int64_t log[14]) {
    if (!c) return HIMUT_ERR_ARG;
    if (!c->norm.have) return fail(c, HIMUT_ERR_ARG, "himut_run_normcounts has not completed");
    const size_t ntri = (size_t)c->ref_K * c->ref_K * c->ref_K;
    for (size_t k = 0; k < ntri; k++) { ccs_tri[k] = (int64_t)c->norm.h_tri[k]; ref_tri[k] = (int64_t)c->norm.h_tri[ntri + k]; }
    for (int k = 0; k < 14; k++) log[k] = (int64_t)c->norm.h_tri[2 * ntri + k];
    return HIMUT_OK;
}

}  // extern "C"
