// libhimut_hip.so: the transcription-strand spectrum (himut_set_strands, himut_sbs384_counts, himut_strand_tricounts,
// himut_strand_callable) over the kernels of himut_strands.h.  The segment list is the context's own and lives until the
// next himut_set_strands or himut_set_reference; every other device buffer is one of the context's scratch pools.  None of
// the calls reads or changes the site sets, parameters, regions or reads; himut_strand_callable reads what the last
// completed callable run left (the map, its offsets, the copies of its chunk list: himut_ctx::Callmap).
#include <hip/hip_runtime.h>

#include "himut_ctx.h"
#include "himut_strands.h"

using namespace himut;

namespace {

constexpr unsigned STRANDS_MAX_WGS = 2048;      // the grids' cap: the kernels stride over what is longer (himut_debug_spectra)

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

inline unsigned strands_grid(const himut_ctx* c, int64_t blocks) {
    const unsigned cap = c->dbg_spectra_wgs > 0 ? (unsigned)c->dbg_spectra_wgs : STRANDS_MAX_WGS;
    return (unsigned)std::min<int64_t>(std::max<int64_t>(blocks, 1), cap);
}

// the reference string and the segment list of it, or the message
int need_segments(himut_ctx* c, const char* who) {
    if (c->reflen <= 0) return fail(c, HIMUT_ERR_ARG, "himut_set_reference has not been called");
    if (c->strands.n <= 0) return fail(c, HIMUT_ERR_ARG, std::string(who) + ": himut_set_strands has not been called for this reference string");
    return HIMUT_OK;
}

StrandSegs segments_of(const himut_ctx* c) {
    StrandSegs S;
    S.start = c->strands.d_start.as<int32_t>(); S.mask = c->strands.d_mask.as<uint8_t>(); S.n = c->strands.n;
    return S;
}

// the bins the kernel left at d_out into out, and the device time into the run's statistics
void finish_counts(himut_ctx* c, const unsigned long long* d_out, int64_t* out, int nbins) {
    unsigned long long h[SBS384_BINS];
    HCHECK(hipMemcpyAsync(h, d_out, (size_t)nbins * 8, hipMemcpyDeviceToHost, c->stream));
    HCHECK(hipStreamSynchronize(c->stream));
    HCHECK(hipGetLastError());
    for (int k = 0; k < nbins; k++) out[k] = (int64_t)h[k];
    memset(&c->stats, 0, sizeof(c->stats));
    c->stats.ms_total = elapsed_ms(c, EV_START, EV_FINAL);
}

}  // namespace

extern "C" {

int himut_set_strands(himut_ctx* c, const int32_t* seg_start, const uint8_t* seg_mask, int64_t n_seg) {
    if (!c) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int {
        if (c->reflen <= 0) return fail(c, HIMUT_ERR_ARG, "himut_set_reference has not been called");
        if (n_seg < 1 || !seg_start || !seg_mask) return fail(c, HIMUT_ERR_ARG, "himut_set_strands: a segment list has at least one segment");
        if (seg_start[0] != 0) return fail(c, HIMUT_ERR_ARG, "himut_set_strands: the first segment starts at 0");
        for (int64_t k = 0; k < n_seg; k++) {
            const std::string who = "himut_set_strands: segment " + std::to_string(k);
            if (k > 0 && seg_start[k] <= seg_start[k - 1]) return fail(c, HIMUT_ERR_ARG, who + " does not start behind the one before it");
            if ((int64_t)seg_start[k] >= c->reflen) return fail(c, HIMUT_ERR_ARG, who + " starts behind the reference string");
            if (seg_mask[k] > 3) return fail(c, HIMUT_ERR_ARG, who + " has a mask above 3");
        }
        HCHECK(hipSetDevice(c->device));
        c->strands.n = 0;
        upload(c->strands.d_start, seg_start, (size_t)n_seg, c->stream);
        upload(c->strands.d_mask, seg_mask, (size_t)n_seg, c->stream);
        HCHECK(hipStreamSynchronize(c->stream));
        c->strands.n = n_seg;
        return HIMUT_OK;
    });
}

int himut_sbs384_counts(himut_ctx* c, const int32_t* pos0, const uint8_t* ref, const uint8_t* alt, int64_t n, uint16_t* cls,
                        int64_t out[387]) {
    if (!c) return HIMUT_ERR_ARG;
    if (!out || n < 0 || (n && (!pos0 || !ref || !alt))) return fail(c, HIMUT_ERR_ARG, "himut_sbs384_counts: bad argument");
    return guarded(c, [&]() -> int {
        if (const int rc = need_segments(c, "himut_sbs384_counts")) return rc;
        HCHECK(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        const size_t nn = (size_t)std::max<int64_t>(n, 1);
        // d_tmp: positions, classes; d_tmp2: ref, alt, the bins
        const size_t o_cls = align256(nn * 4), o_alt = align256(nn), o_out = 2 * o_alt;
        c->d_tmp.reserve(o_cls + nn * 2 + 256);
        c->d_tmp2.reserve(o_out + SBS384_BINS * 8 + 256);
        int32_t* d_pos = c->d_tmp.as<int32_t>();
        uint16_t* d_cls = reinterpret_cast<uint16_t*>(c->d_tmp.as<uint8_t>() + o_cls);
        uint8_t* d_ref = c->d_tmp2.as<uint8_t>();
        uint8_t* d_alt = d_ref + o_alt;
        unsigned long long* d_out = reinterpret_cast<unsigned long long*>(d_ref + o_out);
        if (n) {
            HCHECK(hipMemcpyAsync(d_pos, pos0, (size_t)n * 4, hipMemcpyHostToDevice, st));
            HCHECK(hipMemcpyAsync(d_ref, ref, (size_t)n, hipMemcpyHostToDevice, st));
            HCHECK(hipMemcpyAsync(d_alt, alt, (size_t)n, hipMemcpyHostToDevice, st));
        }
        HCHECK(hipMemsetAsync(d_out, 0, SBS384_BINS * 8, st));
        HCHECK(hipEventRecord(c->ev[EV_START], st));
        if (n)
            hipLaunchKernelGGL(k_sbs384, dim3(strands_grid(c, blocks_for(n, 256))), dim3(256), 0, st, c->d_refseq.as<uint8_t>(), c->reflen,
                               segments_of(c), d_pos, d_ref, d_alt, n, cls ? d_cls : nullptr, d_out);
        HCHECK(hipEventRecord(c->ev[EV_FINAL], st));
        if (n && cls) HCHECK(hipMemcpyAsync(cls, d_cls, (size_t)n * 2, hipMemcpyDeviceToHost, st));
        finish_counts(c, d_out, out, SBS384_BINS);
        c->stats.n_candidates = n;
        return HIMUT_OK;
    });
}

int himut_strand_tricounts(himut_ctx* c, int64_t out[128]) {
    if (!c) return HIMUT_ERR_ARG;
    if (!out) return fail(c, HIMUT_ERR_ARG, "himut_strand_tricounts: bad argument");
    return guarded(c, [&]() -> int {
        if (const int rc = need_segments(c, "himut_strand_tricounts")) return rc;
        HCHECK(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        c->d_tmp2.reserve(ST_BINS * 8 + 256);
        unsigned long long* d_out = c->d_tmp2.as<unsigned long long>();
        HCHECK(hipMemsetAsync(d_out, 0, ST_BINS * 8, st));
        HCHECK(hipEventRecord(c->ev[EV_START], st));
        hipLaunchKernelGGL(k_strand_tricounts, dim3(strands_grid(c, (c->reflen + ST_TILE - 1) / ST_TILE)), dim3(256), 0, st,
                           c->d_refseq.as<uint8_t>(), c->reflen, segments_of(c), d_out);
        HCHECK(hipEventRecord(c->ev[EV_FINAL], st));
        finish_counts(c, d_out, out, ST_BINS);
        c->stats.positions = c->reflen;
        return HIMUT_OK;
    });
}

int himut_strand_callable(himut_ctx* c, int64_t pos[128], int64_t bases[128]) {
    if (!c) return HIMUT_ERR_ARG;
    if (!pos || !bases) return fail(c, HIMUT_ERR_ARG, "himut_strand_callable: bad argument");
    return guarded(c, [&]() -> int {
        himut_ctx::Callmap& M = c->callmap;
        if (!M.have || !M.last_ok) return fail(c, HIMUT_ERR_ARG, "himut_strand_callable: no completed himut_run_callable to read the map of");
        if (c->reflen != M.g_reflen) return fail(c, HIMUT_ERR_ARG, "himut_strand_callable: the reference string is not as long as the one the callable run saw");
        if (const int rc = need_segments(c, "himut_strand_callable")) return rc;
        HCHECK(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        const int64_t nch = (int64_t)M.g_cs.size();
        // d_tmp: the chunks' starts and ends; d_tmp2: the bins
        const size_t o_ce = align256((size_t)std::max<int64_t>(nch, 1) * 4);
        c->d_tmp.reserve(2 * o_ce + 256);
        c->d_tmp2.reserve(2 * ST_BINS * 8 + 256);
        int32_t* d_cs = c->d_tmp.as<int32_t>();
        int32_t* d_ce = reinterpret_cast<int32_t*>(c->d_tmp.as<uint8_t>() + o_ce);
        unsigned long long* d_out = c->d_tmp2.as<unsigned long long>();
        if (nch) {
            HCHECK(hipMemcpyAsync(d_cs, M.g_cs.data(), (size_t)nch * 4, hipMemcpyHostToDevice, st));
            HCHECK(hipMemcpyAsync(d_ce, M.g_ce.data(), (size_t)nch * 4, hipMemcpyHostToDevice, st));
        }
        HCHECK(hipMemsetAsync(d_out, 0, 2 * ST_BINS * 8, st));
        HCHECK(hipEventRecord(c->ev[EV_START], st));
        if (M.n_pos > 0) {
            IvGeo G;
            G.cs = d_cs; G.ce = d_ce; G.mapoff = M.d_mapoff.as<int64_t>(); G.nch = nch; G.ordered = 0;
            G.mstate = M.d_state.as<uint8_t>(); G.mbases = M.d_bases.as<uint16_t>();
            G.refseq = c->d_refseq.as<uint8_t>(); G.reflen = c->reflen;
            hipLaunchKernelGGL(k_strand_callable, dim3(strands_grid(c, blocks_for(M.n_pos, 256 * IV_PER))), dim3(256), 0, st, G,
                               segments_of(c), M.n_pos, d_out);
        }
        HCHECK(hipEventRecord(c->ev[EV_FINAL], st));
        int64_t h[2 * ST_BINS];
        static_assert(2 * ST_BINS <= SBS384_BINS, "finish_counts' host block holds both histograms");
        finish_counts(c, d_out, h, 2 * ST_BINS);
        memcpy(pos, h, ST_BINS * 8);
        memcpy(bases, h + ST_BINS, ST_BINS * 8);
        c->stats.positions = M.n_pos;
        return HIMUT_OK;
    });
}

}  // extern "C"
