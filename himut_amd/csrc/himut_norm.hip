// libhimut_hip.so: normcounts (himut_run_normcounts) over the kernels of himut_norm.h and himut_normq.h, and the
// resident reference string it sweeps (himut_set_reference).
#include <hip/hip_runtime.h>

#include "himut_ctx.h"
#include "himut_normq.h"

using namespace himut;

namespace {

int do_normcounts(himut_ctx* c, const uint8_t* alt_order, int non_human, bool force_tile = false, int attempt = 0) {
    if (int rc = check_scan_inputs(c, true)) return rc;
    const bool phase = c->params.p.phase != 0;
    for (int k = 0; k < 12; k++) if (alt_order[k] > 3) return fail(c, HIMUT_ERR_ARG, "alt_order holds alleles 0..3");
    HCHECK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    c->norm.have = false;
    memset(&c->stats, 0, sizeof(c->stats));
    c->params.unique_qnames = c->unique_qnames ? 1 : 0;

    if (c->cstart.size() > 65535) return fail(c, HIMUT_ERR_ARG, "more than 65,535 chunks in one contig (the sweep's grids take a chunk per row)");
    ChunkTables T = upload_chunks(c, c->cstart, c->cend);
    alloc_derived(c);
    Reads R = make_reads(c);
    Derived D = make_derived(c);
    Chunks C = make_chunks(c, T.n);
    if (phase) c->d_hap.reserve((size_t)T.npairs + 64);
    Phase H = make_phase(c);
    Scalars* sc = borrow_scalars(c);
    const int K = c->ref_K;
    const size_t ntri = (size_t)K * K * K;
    c->norm.d_tri.reserve((2 * ntri + 16) * 8);
    c->norm.d_live.reserve((size_t)c->n + 64);
    const size_t cwords = (size_t)(c->bq_bytes >> 5) + 64;
    c->norm.d_callable.reserve(cwords * 4);
    // the sweep: k_norm_quad (a wave per 256 columns), k_norm_dirty for the positions it lists, k_norm_tile for the tiles it
    // lists; the whole contig with k_norm_tile when one of the two lists was too short (force_tile), or when a test asks
    const bool sweep_tile = force_tile || c->norm.dbg_sweep == 1;
    const bool sweep_quad = !sweep_tile;
    // the sweep's grid (workgroups of NQ_WAVES waves, a wave per 256 positions; NQ_Q workgroups per XCD class and chunk)
    int32_t maxspan = 1;
    for (size_t k = 0; k < c->cstart.size(); k++) maxspan = std::max(maxspan, c->cend[k] - c->cstart[k]);
    const int64_t q_per = ((int64_t)blocks_for(maxspan, NQ_WG_COLS) + 7) / 8;             // workgroup tiles of a chunk per XCD class
    // (NQ_Q workgroups per class and chunk keep a wave on a dozen tiles of a long contig; a contig of a few chunks gets
    //  more of them, so that the grid still fills the chip: about 4096 workgroups where the tiles allow)
    const int64_t q_want = std::max<int64_t>(NQ_Q, (4096 + 8 * std::max<int64_t>(T.n, 1) - 1) / (8 * std::max<int64_t>(T.n, 1)));
    const unsigned q_gx = 8u * (unsigned)std::min<int64_t>(q_want, q_per);
    const int64_t q_regions = (int64_t)q_gx * (int64_t)std::max<int64_t>(T.n, 1);
    // The sweep's scratch, laid out by each chunk's own length (phase blocks range from one position to megabases): tile k
    // of chunk j is row toff[j] + k of the plan, and workgroup x of chunk j lists the positions it leaves to k_norm_dirty
    // in entries [doff[q_gx j + x], doff[q_gx j + x + 1]) of one list.  A part has room for a quarter of the positions its
    // workgroup sweeps and some slack (a column with another allele is one in thirty), never for more than all of them;
    // after a pass that ran out, for the density that pass needed (dirty_room: entries per NQ_WG_COLS positions).
    // (the table is built and uploaded again only when the chunks, the room or the test's cap changed: a contig's passes
    //  over the same chunks reuse it)
    const int64_t n_ch = T.n, G = q_gx / 8;
    const int64_t dbg_cap = c->norm.dbg_dirty_cap > 0 && attempt == 0 ? c->norm.dbg_dirty_cap : 0;   // (tests: the first pass overflows)
    std::vector<int64_t>& lay = c->norm.h_lay;
    std::vector<int64_t>& swept = c->norm.h_swept;                                      // positions per workgroup
    auto part_cap = [&](int64_t n) {
        int64_t cap = n / 4 + std::min<int64_t>(64, n / 4 + 8);
        if (c->norm.dirty_room > 0) cap = std::max(cap, (n * c->norm.dirty_room + NQ_WG_COLS - 1) / NQ_WG_COLS + 8);
        return std::min(cap, n);
    };
    if (!(c->norm.lay_ok && c->norm.lay_room == c->norm.dirty_room && c->norm.lay_dbg == dbg_cap && c->norm.lay_cs == c->cstart &&
          c->norm.lay_ce == c->cend)) {
        lay.assign((size_t)(n_ch + 1 + q_regions + 1), 0);
        swept.assign((size_t)q_regions, 0);
        int64_t* toff = lay.data();
        int64_t* doff = toff + n_ch + 1;
        for (int64_t k = 0; k < n_ch; k++) {
            const int64_t len = std::max<int64_t>((int64_t)c->cend[k] - c->cstart[k], 0);
            toff[k + 1] = toff[k] + (len + NQ_COLS - 1) / NQ_COLS;
            const int64_t per = std::min<int64_t>(q_per, ((len + NQ_WG_COLS - 1) / NQ_WG_COLS + 7) / 8);   // (k_norm_quad's mapping)
            for (int64_t x = 0; x < (int64_t)q_gx; x++) {
                int64_t n = 0;
                for (int64_t t = x >> 3; t < per; t += G)
                    n += std::min<int64_t>(std::max<int64_t>(len - ((x & 7) * per + t) * NQ_WG_COLS, 0), NQ_WG_COLS);
                swept[(size_t)(k * q_gx + x)] = n;
            }
        }
        for (int64_t r = 0; r < q_regions; r++) {
            const int64_t cap = part_cap(swept[(size_t)r]);
            doff[r + 1] = doff[r] + (dbg_cap > 0 ? std::min(cap, dbg_cap) : cap);
        }
        upload(c->norm.d_lay, lay.data(), lay.size(), st);
        c->norm.lay_ok = true; c->norm.lay_room = c->norm.dirty_room; c->norm.lay_dbg = dbg_cap;
        c->norm.lay_cs = c->cstart; c->norm.lay_ce = c->cend;
    }
    const int64_t* toff = lay.data();
    const int64_t* doff = toff + n_ch + 1;
    const int64_t n_tiles = toff[n_ch], n_dirty = doff[q_regions];
    // tiles left to k_norm_tile (more pieces than the plan holds, more columns with another allele than a wave's pool): room for
    // every tile of the contig
    const unsigned redo_cap = (unsigned)std::min<int64_t>(n_tiles + 64, (int64_t)1 << 28);
    if (sweep_quad) {
        c->norm.d_dirty.reserve((size_t)n_dirty * sizeof(NormDirty) + 256);
        c->norm.d_dcount.reserve((size_t)q_regions * 4 + 256);
        c->norm.d_redo.reserve((size_t)redo_cap * sizeof(NormRedo) + 256);
    }

    HCHECK(hipEventRecord(c->ev[EV_START], st));
    flag_bases_once(c, st);
    HCHECK(hipMemsetAsync(sc, 0, sizeof(Scalars), st));
    HCHECK(hipMemsetAsync(c->d_ccs.p, 0, (size_t)c->n + 1, st));
    HCHECK(hipMemsetAsync(c->norm.d_tri.p, 0, (2 * ntri + 16) * 8, st));
    // (d_callable is not cleared: k_callable writes the words of every read)
    if (c->n > 0) run_parse_stage(c, R, D, sc);   // (the quality sums are k_callable's)
    else stage_event(c, EV_PARSE, 2, st);
    int32_t maxend = 0;
    for (int32_t e : c->cend) maxend = std::max(maxend, e);
    const int64_t nblk = ((int64_t)maxend >> WIN_SHIFT) + 2;
    c->d_winlo.reserve((size_t)nblk * 4 + 64);
    c->d_winhi.reserve((size_t)nblk * 4 + 64);
    if (c->n > 0 && T.n > 0) {
        hipLaunchKernelGGL(k_read_live, dim3(blocks_for(c->n, 16)), dim3(256), 0, st, R, D, C, c->params,
                           c->norm.d_live.as<uint8_t>(), c->d_ccs.as<uint8_t>(), &sc->err);
        // (k_callable takes the reads with a low mean quality out of `live`: before the phased runs' count of the reads)
        hipLaunchKernelGGL(k_callable, dim3(blocks_for(c->n, 4)), dim3(256), 0, st, R, D, c->params, c->norm.d_live.as<uint8_t>(),
                           c->norm.d_callable.as<uint32_t>(), c->d_ccs.as<uint8_t>());
        if (phase && T.npairs > 0) {
            launch_read_hap(c, R, D, C, H, T, sc);
            hipLaunchKernelGGL(k_pair_ccs, dim3(blocks_for(T.npairs, 256)), dim3(256), 0, st, C, H, R, c->norm.d_live.as<uint8_t>(),
                               T.npairs, c->d_ccs.as<uint8_t>());
        }
        launch_window_index(c, R, nblk, st);
    }
    HCHECK(hipEventRecord(c->ev[EV_EMIT], st));

    NormArgs A;
    A.P = c->params;
    A.S.pon = c->d_pon.as<uint64_t>(); A.S.npon = c->npon; A.S.com = c->d_com.as<uint64_t>(); A.S.ncom = c->ncom;
    A.S.posbits = c->d_posbits.as<uint32_t>(); A.S.nposbits = c->nposbits;
    A.lut = c->d_lut.as<GtLut>();
    A.R = R; A.C = C; A.H = H;
    A.refseq = c->d_refseq.as<uint8_t>(); A.reflen = c->reflen;
    memcpy(A.cls, c->ref_cls, 256);
    A.K = K; A.cA = c->ref_cls['A']; A.cC = c->ref_cls['C']; A.cG = c->ref_cls['G']; A.cT = c->ref_cls['T'];
    memcpy(A.alt_order, alt_order, 12);
    A.non_human = non_human;
    A.ccs_tri = c->norm.d_tri.as<unsigned long long>(); A.ref_tri = A.ccs_tri + ntri; A.log = A.ccs_tri + 2 * ntri;
    A.err = &sc->err;
    if (c->n > 0 && T.n > 0) {
        A.X = PosIndex{}; A.colstore = nullptr; A.p_lo = 0; A.p_hi = 0;
        if (sweep_quad) {
            // the plan: which pieces of which reads lie over each tile of 256 positions (k_norm_plan), then the sweep
            const int64_t tpc = (int64_t)blocks_for(maxspan, NQ_COLS);                  // tiles of the longest chunk (the grid)
            c->norm.d_plan.reserve((size_t)n_tiles * NQ_ITEMS * sizeof(NqItem) + 256);
            c->norm.d_plancnt.reserve((size_t)n_tiles * 4 + 256);
            const int64_t* d_toff = c->norm.d_lay.as<int64_t>();
            const int64_t* d_doff = d_toff + n_ch + 1;
            const dim3 pgrid((unsigned)blocks_for(blocks_for(tpc, NQ_PLAN_TILES), 4), (unsigned)T.n);
            hipLaunchKernelGGL(phase ? k_norm_plan<true> : k_norm_plan<false>, pgrid, dim3(256), 0, st, A, D, c->d_winlo.as<int32_t>(),
                               c->d_winhi.as<int32_t>(), nblk, d_toff, c->norm.d_plan.as<NqItem>(), c->norm.d_plancnt.as<uint32_t>(),
                               c->norm.d_redo.as<NormRedo>(), &sc->nredo, redo_cap);
            const dim3 grid(q_gx, (unsigned)T.n);
            stage_event(c, EV_INDEX, 1, st);                                            // (around k_norm_quad: stats.ms_capture)
            const unsigned pool_limit = c->norm.dbg_pool > 0 ? (unsigned)std::min(c->norm.dbg_pool, NQ_SLOTS) : (unsigned)NQ_SLOTS;
            hipLaunchKernelGGL(phase ? k_norm_quad<true> : k_norm_quad<false>, grid, dim3(NQ_WAVES * 64), 0, st, A,
                               c->norm.d_callable.as<uint32_t>(), (int64_t)c->bq_bytes, c->norm.d_refcode.as<uint16_t>(),
                               c->norm.d_plan.as<NqItem>(), c->norm.d_plancnt.as<uint32_t>(), d_toff, q_per, c->norm.d_dirty.as<NormDirty>(),
                               d_doff, c->norm.d_dcount.as<uint32_t>(), &sc->dirty_over, c->norm.d_redo.as<NormRedo>(),
                               &sc->nredo, redo_cap, pool_limit);
            stage_event(c, EV_GATHER, 1, st);
            hipLaunchKernelGGL(k_norm_dirty, dim3((unsigned)std::min<int64_t>(blocks_for(q_regions, 4), 16384)), dim3(256), 0, st, A,
                               c->norm.d_dirty.as<NormDirty>(), c->norm.d_dcount.as<uint32_t>(), d_doff, q_regions);
            // (returns at once unless a tile was listed)
            hipLaunchKernelGGL(k_norm_tile, dim3(1024), dim3(256), 0, st, A, D, c->norm.d_callable.as<uint32_t>(), c->d_winlo.as<int32_t>(),
                               c->d_winhi.as<int32_t>(), nblk, (int64_t)0, c->norm.d_redo.as<NormRedo>(), &sc->nredo, redo_cap);
        } else {
            const int64_t per = ((int64_t)blocks_for(maxspan, 256) + 7) / 8;
            const dim3 grid(8u * (unsigned)std::min<int64_t>(NT_Q, per), (unsigned)T.n);
            hipLaunchKernelGGL(k_norm_tile, grid, dim3(256), 0, st, A, D, c->norm.d_callable.as<uint32_t>(), c->d_winlo.as<int32_t>(),
                               c->d_winhi.as<int32_t>(), nblk, per, (const NormRedo*)nullptr, (const unsigned int*)nullptr, 0u);
        }
    }
    if (c->n > 0 && T.n > 0)
        launch_count_flags(c, sc);
    HCHECK(hipEventRecord(c->ev[EV_FINAL], st));
    c->norm.h_tri.assign(2 * ntri + 16, 0ULL);
    Scalars hs;
    HCHECK(hipMemcpyAsync(c->norm.h_tri.data(), c->norm.d_tri.p, (2 * ntri + 16) * 8, hipMemcpyDeviceToHost, st));
    HCHECK(hipMemcpyAsync(&hs, sc, sizeof(Scalars), hipMemcpyDeviceToHost, st));
    HCHECK(hipStreamSynchronize(st));
    // The list of positions left to k_norm_dirty was too short in some part (a region where more than one position in four
    // holds another allele: deep piles, a sample far from the reference): the same sweep once more with the room the
    // counters say it needs -- the context keeps it, as a density, for its later passes, as himut_run keeps its capacities
    // (a part that ran out only under the test's cap raises nothing).  The list of tiles was too short (or the room still
    // is, which the counters rule out): the whole contig with k_norm_tile.
    if (hs.dirty_over && !force_tile && attempt == 0 && hs.nredo <= redo_cap) {
        std::vector<uint32_t> need((size_t)q_regions);
        HCHECK(hipMemcpy(need.data(), c->norm.d_dcount.p, (size_t)q_regions * 4, hipMemcpyDeviceToHost));
        int64_t room = c->norm.dirty_room;
        for (int64_t r = 0; r < q_regions; r++) {
            const int64_t v = need[(size_t)r], n = swept[(size_t)r];
            if (n > 0 && v > part_cap(n)) room = std::max(room, ((v + v / 8) * NQ_WG_COLS + n - 1) / n);
        }
        c->norm.dirty_room = room;
        return do_normcounts(c, alt_order, non_human, false, 1);
    }
    if ((hs.dirty_over || hs.nredo > redo_cap) && !force_tile) return do_normcounts(c, alt_order, non_human, true, attempt + 1);
    c->stats.reran = (force_tile || attempt > 0) ? 1 : 0;
    if (hs.err) return check_device_err(c, hs.err);
    c->norm.h_tri[2 * ntri + 0] = hs.nccs;
    c->stats.ms_total = elapsed_ms(c, EV_START, EV_FINAL);
    if (c->timing >= 2) {   // recorded by run_parse_stage only then (an unrecorded event leaves a sticky HIP error)
        c->stats.ms_parse = elapsed_ms(c, EV_START, EV_PARSE);
        c->stats.ms_index = elapsed_ms(c, EV_PARSE, EV_EMIT);       // the read pass: filters, callable bits, window index
    }
    c->stats.ms_eval = elapsed_ms(c, EV_EMIT, EV_FINAL);            // the position sweep: plan, k_norm_quad, k_norm_dirty, listed tiles
    if (c->timing >= 1 && sweep_quad && c->n > 0 && T.n > 0)
        c->stats.ms_capture = elapsed_ms(c, EV_INDEX, EV_GATHER);   // k_norm_quad by itself, the pass's dominant kernel
    c->stats.n_reads = c->n; c->stats.read_bases = c->read_bases; c->stats.positions = T.positions;
    c->stats.column_slots = hs.nredo;        // (normcounts: tiles k_norm_quad left to k_norm_tile)
    c->norm.have = true;
    return HIMUT_OK;
}

}  // namespace

extern "C" {

int himut_set_reference(himut_ctx* c, const uint8_t* seq, int64_t len, const uint8_t* cls, int n_classes) {
    if (!c) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int {
        if (!seq || len <= 0 || !cls || n_classes < 5 || n_classes > 32) return fail(c, HIMUT_ERR_ARG, "bad reference / class table");
        HCHECK(hipSetDevice(c->device));
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
    if (!c || sweep < 0 || sweep > 1 || dirty_cap < 0 || pool_slots < 0) return HIMUT_ERR_ARG;
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

int himut_get_normcounts(himut_ctx* c, int64_t* ccs_tri, int64_t* ref_tri, int64_t log[14]) {
    if (!c) return HIMUT_ERR_ARG;
    if (!c->norm.have) return fail(c, HIMUT_ERR_ARG, "himut_run_normcounts has not completed");
    const size_t ntri = (size_t)c->ref_K * c->ref_K * c->ref_K;
    for (size_t k = 0; k < ntri; k++) { ccs_tri[k] = (int64_t)c->norm.h_tri[k]; ref_tri[k] = (int64_t)c->norm.h_tri[ntri + k]; }
    for (int k = 0; k < 14; k++) log[k] = (int64_t)c->norm.h_tri[2 * ntri + k];
    return HIMUT_OK;
}

}  // extern "C"
