// libhimut_hip.so: the dense pile of himut_pile_counts (himut_pile.h), behind the cs decode alone (run_parse_stage,
// himut_front.hip): a diagnostic export, the pile of every position of a range as the call run's columns hold it.
#include <hip/hip_runtime.h>

#include "himut_ctx.h"
#include "himut_pile.h"

using namespace himut;

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

}  // namespace

extern "C" {

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
