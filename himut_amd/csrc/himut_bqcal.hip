// libhimut_hip.so: the bqcal run (himut_run_bqcal, himut_get_bqcal) over the kernels of himut_bqcal.h.  The cs decode in
// front of it is the read pass every pipeline starts with (run_parse_stage, himut_front.hip), under a parameter block of
// the run's own; the regions become tiles here, not through upload_chunks: the chunk tables of the call run stay as they are.
#include <hip/hip_runtime.h>

#include "himut_ctx.h"
#include "himut_bqcal.h"

using namespace himut;

extern "C" {

int himut_run_bqcal(himut_ctx* c, const himut_bqcal_params* p) {
    if (!c) return HIMUT_ERR_ARG;
    if (!p) return fail(c, HIMUT_ERR_ARG, "himut_run_bqcal: bad argument");
    return guarded(c, [&]() -> int {
        // (a region's start > end is found below, region by region, with its place in the reference)
        if (int rc = check_run_inputs(c, NEED_LUT | NEED_READS | NEED_REGIONS | NEED_REFERENCE)) return rc;
        const int64_t nreg = (int64_t)c->cstart.size();
        std::vector<int64_t> tileoff((size_t)nreg + 1, 0);
        int64_t positions = 0;
        for (int64_t k = 0; k < nreg; k++) {
            const int64_t s = c->cstart[(size_t)k], e = c->cend[(size_t)k];
            if (s > e) return fail(c, HIMUT_ERR_CHUNK, "ValueError: invalid coordinates: region start > end");
            if (s < 0 || e > c->reflen) return fail(c, HIMUT_ERR_CHUNK, "IndexError: region outside the reference string");
            tileoff[(size_t)k + 1] = tileoff[(size_t)k] + (e - s + BQ_TP - 1) / BQ_TP;
            positions += e - s;
        }
        const int64_t n_tiles = tileoff[(size_t)nreg];
        // the regions by start, with the running maximum of their ends: which reads some region fetches (k_bqcal_bases)
        std::vector<int32_t> sstart, spmax;
        sorted_regions(c->cstart, c->cend, &sstart, &spmax);

        HCHECK(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        himut_ctx::Bqcal& B = c->bqcal;
        memset(B.out, 0, sizeof(B.out));
        memset(&c->stats, 0, sizeof(c->stats));
        // resident workgroups: two per CU (the kernel's LDS), a multiple of eight so that a workgroup's tiles stay on its XCD's range
        const int64_t resident = std::max<int64_t>(8, (int64_t)c->n_cus * 2 / 8 * 8);
        const unsigned nwg = (unsigned)std::max<int64_t>(1, std::min(n_tiles, resident));

        alloc_derived(c);
        upload(B.d_rstart, c->cstart, st); upload(B.d_rend, c->cend, st); upload(B.d_tileoff, tileoff, st);
        upload(B.d_sstart, sstart, st); upload(B.d_spmax, spmax, st);
        B.d_tiles.reserve((size_t)std::max<int64_t>(n_tiles, 1) * sizeof(BqTile));
        B.d_part.reserve((size_t)nwg * BQ_ROW * 8);
        B.d_out.reserve((size_t)BQ_ROW * 8);
        B.d_sc.reserve(sizeof(Scalars));
        Scalars* sc = B.d_sc.as<Scalars>();        // (not the context's: the call and germline runs keep theirs as they left them)
        Scalars hs;
        memset(&hs, 0, sizeof(hs));

        HCHECK(hipEventRecord(c->ev[EV_START], st));
        HCHECK(hipMemsetAsync(sc, 0, sizeof(Scalars), st));
        HCHECK(hipMemsetAsync(B.d_part.p, 0, (size_t)nwg * BQ_ROW * 8, st));
        HCHECK(hipMemsetAsync(B.d_out.p, 0, (size_t)BQ_ROW * 8, st));
        flag_bases_once(c, st);
        // the decode marks nothing (no bitmap); the sweep looks at flag 0x100 and the mapping quality itself
        const Params P = open_gate_params(c, p->min_mapq);
        const Reads R = make_reads(c);
        const Derived D = make_derived(c);
        if (c->n > 0) {
            run_parse_stage(c, R, D, sc, &P);
            hipLaunchKernelGGL(k_bqcal_bases, dim3(blocks_for(c->n, 16)), dim3(256), 0, st, R, D, B.d_sstart.as<int32_t>(),
                               B.d_spmax.as<int32_t>(), nreg, &sc->err);
        } else {
            stage_event(c, EV_PARSE, 2, st);
        }
        if (n_tiles > 0) {
            hipLaunchKernelGGL(k_bqcal_tiles, dim3(blocks_for(n_tiles, 256)), dim3(256), 0, st, R, B.d_rstart.as<int32_t>(),
                               B.d_rend.as<int32_t>(), B.d_tileoff.as<int64_t>(), nreg, n_tiles, B.d_tiles.as<BqTile>());
            BqArgs A;
            A.p = *p; A.lut = c->d_lut.as<GtLut>(); A.R = R; A.D = D; A.refseq = c->d_refseq.as<uint8_t>();
            A.tiles = B.d_tiles.as<BqTile>(); A.n_tiles = n_tiles;
            A.rb = B.dbg_rb > 0 ? std::min(B.dbg_rb, BQ_RB) : BQ_RB;
            A.part = B.d_part.as<unsigned long long>(); A.err = &sc->err;
            hipLaunchKernelGGL(k_bqcal, dim3(nwg), dim3(BQ_NT), 0, st, A);
            stage_event(c, EV_SWEEP, 2, st);
            hipLaunchKernelGGL(k_bqcal_reduce, dim3(blocks_for(BQ_ROW, 256)), dim3(256), 0, st, B.d_part.as<unsigned long long>(),
                               (int64_t)nwg, B.d_out.as<long long>());
        } else {
            stage_event(c, EV_SWEEP, 2, st);
        }
        HCHECK(hipEventRecord(c->ev[EV_FINAL], st));
        int64_t out[BQ_ROW];
        HCHECK(hipMemcpyAsync(out, B.d_out.p, sizeof(out), hipMemcpyDeviceToHost, st));
        HCHECK(hipMemcpyAsync(&hs, sc, sizeof(Scalars), hipMemcpyDeviceToHost, st));
        HCHECK(hipStreamSynchronize(st));
        if (hs.err) return check_device_err(c, hs.err);
        memcpy(B.out, out, sizeof(out));
        c->stats.ms_total = elapsed_ms(c, EV_START, EV_FINAL);
        if (c->timing >= 2) {
            c->stats.ms_parse = elapsed_ms(c, EV_START, EV_PARSE);
            c->stats.ms_eval = elapsed_ms(c, EV_PARSE, EV_SWEEP);
            c->stats.ms_finalize = elapsed_ms(c, EV_SWEEP, EV_FINAL);
        }
        c->stats.n_reads = c->n; c->stats.read_bases = c->read_bases; c->stats.positions = positions;
        return HIMUT_OK;
    });
}

int himut_get_bqcal(himut_ctx* c, int64_t match[256], int64_t mismatch[256], int64_t log[12]) {
    if (!c || !match || !mismatch) return HIMUT_ERR_ARG;
    const himut_ctx::Bqcal& B = c->bqcal;
    memcpy(match, B.out, 256 * sizeof(int64_t));
    memcpy(mismatch, B.out + 256, 256 * sizeof(int64_t));
    if (log) memcpy(log, B.out + 512, 12 * sizeof(int64_t));
    return HIMUT_OK;
}

int himut_debug_bqcal(himut_ctx* c, int row_batch) {
    if (!c || row_batch < 0) return HIMUT_ERR_ARG;
    c->bqcal.dbg_rb = row_batch;
    return HIMUT_OK;
}

}  // extern "C"
