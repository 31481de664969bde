// libhimut_hip.so: the indel and doublet spectra (himut_id83_classify, himut_dbs78_counts) over the kernels of
// himut_spectra.h.  Neither call reads or changes the context's site sets, parameters, regions or reads; the ID83 call
// reads the resident reference string.  Device buffers are the context's scratch pools.
#include <hip/hip_runtime.h>

#include "himut_ctx.h"
#include "himut_spectra.h"

using namespace himut;

namespace {

constexpr unsigned SPECTRA_MAX_WGS = 2048;      // the grid's cap: the kernels stride over longer lists (himut_debug_spectra)

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

inline unsigned spectra_grid(const himut_ctx* c, int64_t n) {
    const unsigned cap = c->dbg_spectra_wgs > 0 ? (unsigned)c->dbg_spectra_wgs : SPECTRA_MAX_WGS;
    return std::min<unsigned>(blocks_for(n, 256), cap);
}

}  // namespace

extern "C" {

int himut_id83_classify(himut_ctx* c, const int32_t* anchor0, const uint8_t* type, const int32_t* len, const uint8_t* bases,
                        int64_t n, uint8_t* cls, int64_t out[88]) {
    if (!c) return HIMUT_ERR_ARG;
    if (!out || n < 0 || (n && (!anchor0 || !type || !len || !bases))) return fail(c, HIMUT_ERR_ARG, "himut_id83_classify: bad argument");
    return guarded(c, [&]() -> int {
        if (c->reflen <= 0) return fail(c, HIMUT_ERR_ARG, "himut_set_reference has not been called");
        for (int64_t i = 0; i < n; i++) {
            if (len[i] < 1 || len[i] > ID83_MAX_LEN)
                return fail(c, HIMUT_ERR_ARG, "himut_id83_classify: allele " + std::to_string(i) + " has a length outside 1..64");
            if (type[i] > 1)
                return fail(c, HIMUT_ERR_ARG, "himut_id83_classify: allele " + std::to_string(i) + " has a type other than 0 (deletion) and 1 (insertion)");
        }
        HCHECK(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        const size_t nn = (size_t)std::max<int64_t>(n, 1);
        // d_tmp: anchors, lengths; d_tmp2: inserted bases (16-byte rows), types, classes, the bins
        const size_t o_len = align256(nn * 4), o_type = align256(nn * 16), o_cls = o_type + align256(nn), o_out = o_cls + align256(nn);
        c->d_tmp.reserve(o_len + nn * 4 + 256);
        c->d_tmp2.reserve(o_out + ID83_BINS * 8 + 256);
        int32_t* d_anchor = c->d_tmp.as<int32_t>();
        int32_t* d_len = reinterpret_cast<int32_t*>(c->d_tmp.as<uint8_t>() + o_len);
        uint8_t* d_bases = c->d_tmp2.as<uint8_t>();
        uint8_t* d_type = d_bases + o_type;
        uint8_t* d_cls = d_bases + o_cls;
        unsigned long long* d_out = reinterpret_cast<unsigned long long*>(d_bases + o_out);
        HCHECK(hipEventRecord(c->ev[EV_SIDE], st));
        if (n) {
            HCHECK(hipMemcpyAsync(d_anchor, anchor0, (size_t)n * 4, hipMemcpyHostToDevice, st));
            HCHECK(hipMemcpyAsync(d_len, len, (size_t)n * 4, hipMemcpyHostToDevice, st));
            HCHECK(hipMemcpyAsync(d_bases, bases, (size_t)n * 16, hipMemcpyHostToDevice, st));
            HCHECK(hipMemcpyAsync(d_type, type, (size_t)n, hipMemcpyHostToDevice, st));
        }
        HCHECK(hipMemsetAsync(d_out, 0, ID83_BINS * 8, st));
        HCHECK(hipEventRecord(c->ev[EV_START], st));
        if (n)
            hipLaunchKernelGGL(k_id83, dim3(spectra_grid(c, n)), dim3(256), 0, st, c->d_refseq.as<uint8_t>(), c->reflen, d_anchor,
                               d_type, d_len, d_bases, n, cls ? d_cls : nullptr, d_out);
        HCHECK(hipEventRecord(c->ev[EV_FINAL], st));
        unsigned long long h[ID83_BINS];
        HCHECK(hipMemcpyAsync(h, d_out, ID83_BINS * 8, hipMemcpyDeviceToHost, st));
        if (n && cls) HCHECK(hipMemcpyAsync(cls, d_cls, (size_t)n, hipMemcpyDeviceToHost, st));
        HCHECK(hipStreamSynchronize(st));
        for (int k = 0; k < ID83_BINS; k++) out[k] = (int64_t)h[k];
        memset(&c->stats, 0, sizeof(c->stats));
        c->stats.ms_total = elapsed_ms(c, EV_START, EV_FINAL);      // himut_get_stats: the kernel alone,
        c->stats.ms_parse = elapsed_ms(c, EV_SIDE, EV_START);       // the upload of the list in front of it
        c->stats.n_candidates = n;
        return HIMUT_OK;
    });
}

int himut_dbs78_counts(himut_ctx* c, const uint8_t* ref2, const uint8_t* alt2, int64_t n, uint8_t* cls, int64_t out[80]) {
    if (!c) return HIMUT_ERR_ARG;
    if (!out || n < 0 || (n && (!ref2 || !alt2))) return fail(c, HIMUT_ERR_ARG, "himut_dbs78_counts: bad argument");
    return guarded(c, [&]() -> int {
        HCHECK(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        const size_t nn = (size_t)std::max<int64_t>(n, 1);
        const size_t o_alt = align256(nn * 2), o_cls = 2 * o_alt, o_out = o_cls + align256(nn);
        c->d_tmp2.reserve(o_out + DBS78_BINS * 8 + 256);
        uint8_t* d_ref = c->d_tmp2.as<uint8_t>();
        uint8_t* d_alt = d_ref + o_alt;
        uint8_t* d_cls = d_ref + o_cls;
        unsigned long long* d_out = reinterpret_cast<unsigned long long*>(d_ref + o_out);
        if (n) {
            HCHECK(hipMemcpyAsync(d_ref, ref2, (size_t)n * 2, hipMemcpyHostToDevice, st));
            HCHECK(hipMemcpyAsync(d_alt, alt2, (size_t)n * 2, hipMemcpyHostToDevice, st));
        }
        HCHECK(hipMemsetAsync(d_out, 0, DBS78_BINS * 8, st));
        if (n)
            hipLaunchKernelGGL(k_dbs78, dim3(spectra_grid(c, n)), dim3(256), 0, st, d_ref, d_alt, n, cls ? d_cls : nullptr, d_out);
        unsigned long long h[DBS78_BINS];
        HCHECK(hipMemcpyAsync(h, d_out, DBS78_BINS * 8, hipMemcpyDeviceToHost, st));
        if (n && cls) HCHECK(hipMemcpyAsync(cls, d_cls, (size_t)n, hipMemcpyDeviceToHost, st));
        HCHECK(hipStreamSynchronize(st));
        for (int k = 0; k < DBS78_BINS; k++) out[k] = (int64_t)h[k];
        return HIMUT_OK;
    });
}

int himut_debug_spectra(himut_ctx* c, int max_workgroups) {
    if (!c || max_workgroups < 0) return HIMUT_ERR_ARG;
    c->dbg_spectra_wgs = max_workgroups;
    return HIMUT_OK;
}

}  // extern "C"
