// libhimut_hip.so: the mutation-pattern counts over the kernels of himut_fasta.h (trinucleotides of the resident
// string or of FASTA text, SBS96 / SBS1536) and the phase edges of himut_edges.h.
#include <hip/hip_runtime.h>

#include "himut_ctx.h"
#include "himut_fasta.h"
#include "himut_edges.h"

using namespace himut;

namespace {

// reflib.get_chrom_tricount of `n` bytes of FASTA text on the device (k_fasta_tricounts): `tail` holds the first two
// letters behind them (none for a whole record or the resident string), the counts are added to out[64]
constexpr int64_t FASTA_WINDOW = 64 << 20;       // staging window of himut_fasta_tricounts (himut_debug_fasta_window)
void launch_fasta_tricounts(const uint8_t* p, int64_t n, uint32_t tail, unsigned long long* out, hipStream_t st) {
    if (n <= 0) return;
    const int64_t tiles = (n + FASTA_TILE - 1) / FASTA_TILE;
    hipLaunchKernelGGL(k_fasta_tricounts, dim3((unsigned)std::min<int64_t>(tiles, 2048)), dim3(256), 0, st, p, n, tail, out);
}

// mutlib.load_sbs96_counts (R = 1) / load_sbs1536_counts (R = 2) of the resident string: NB = 6 * 4^(2R) + 3 bins
template <int R>
int sbs_counts(himut_ctx* c, const int32_t* pos0, const uint8_t* ref, const uint8_t* alt, int64_t n, int64_t* out) {
    constexpr int NB = SbsBins<R>::total;
    if (!c || !out || n < 0 || (n && (!pos0 || !ref || !alt))) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int {
        if (c->reflen <= 0) return fail(c, HIMUT_ERR_ARG, "himut_set_reference has not been called");
        HCHECK(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        const size_t nn = (size_t)std::max<int64_t>(n, 1);
        c->d_tmp.reserve(nn * 4 + 256);
        c->d_tmp2.reserve(nn * 2 + NB * 8 + 512);
        uint8_t* d_ref = c->d_tmp2.as<uint8_t>();
        uint8_t* d_alt = d_ref + nn;
        unsigned long long* d_out = reinterpret_cast<unsigned long long*>(c->d_tmp2.as<uint8_t>() + ((2 * nn + 255) & ~(size_t)255));
        if (n) {
            HCHECK(hipMemcpyAsync(c->d_tmp.p, pos0, (size_t)n * 4, hipMemcpyHostToDevice, st));
            HCHECK(hipMemcpyAsync(d_ref, ref, (size_t)n, hipMemcpyHostToDevice, st));
            HCHECK(hipMemcpyAsync(d_alt, alt, (size_t)n, hipMemcpyHostToDevice, st));
        }
        HCHECK(hipMemsetAsync(d_out, 0, NB * 8, st));
        if (n)
            hipLaunchKernelGGL(k_sbs<R>, dim3(std::min<unsigned>(blocks_for(n, 256), 2048u)), dim3(256), 0, st, c->d_refseq.as<uint8_t>(),
                               c->reflen, c->d_tmp.as<int32_t>(), d_ref, d_alt, n, d_out);
        std::vector<unsigned long long> h(NB);
        HCHECK(hipMemcpyAsync(h.data(), d_out, NB * 8, hipMemcpyDeviceToHost, st));
        HCHECK(hipStreamSynchronize(st));
        for (int k = 0; k < NB; k++) out[k] = (int64_t)h[k];
        return HIMUT_OK;
    });
}

}  // namespace

extern "C" {

int himut_run_edges(himut_ctx* c, const int32_t* hpos, const uint8_t* href, int64_t n_het, int min_bq, int min_mapq,
                    int64_t band, uint32_t* counts) {
    if (!c || !counts || band < 1 || n_het < 0 || (n_het && (!hpos || !href))) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int {
        if (!c->have_reads) return fail(c, HIMUT_ERR_ARG, "himut_push_reads has not been called");
        if (!c->have_params) return fail(c, HIMUT_ERR_ARG, "himut_set_params has not been called");   // the cs decode reads them
        HCHECK(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        alloc_derived(c);
        Reads R = make_reads(c);
        Derived D = make_derived(c);
        Scalars* sc = borrow_scalars(c);
        const size_t nc = (size_t)std::max<int64_t>(n_het, 1) * (size_t)band * 4;
        c->d_tmp.reserve(nc * 4 + 256);
        upload(c->d_hpos, hpos, (size_t)n_het, st);
        upload(c->d_href, href, (size_t)n_het, st);
        HCHECK(hipEventRecord(c->ev[EV_START], st));
        HCHECK(hipMemsetAsync(sc, 0, sizeof(Scalars), st));
        HCHECK(hipMemsetAsync(c->d_tmp.p, 0, nc * 4, st));
        if (c->n > 0) {
            run_parse_stage(c, R, D, sc);
            if (n_het >= 2)
                hipLaunchKernelGGL(k_edges, dim3(blocks_for(c->n, 4)), dim3(256), 0, st, R, D, c->d_hpos.as<int32_t>(),
                                   c->d_href.as<uint8_t>(), n_het, min_bq, min_mapq, band, c->d_tmp.as<uint32_t>(), &sc->err);
        }
        HCHECK(hipEventRecord(c->ev[EV_FINAL], st));
        Scalars hs;
        HCHECK(hipMemcpyAsync(counts, c->d_tmp.p, nc * 4, hipMemcpyDeviceToHost, st));
        HCHECK(hipMemcpyAsync(&hs, sc, sizeof(Scalars), hipMemcpyDeviceToHost, st));
        HCHECK(hipStreamSynchronize(st));
        c->have_phase = false;        // d_hpos / d_href, the phase sets' arrays, were reused (a phased run needs himut_set_phase again)
        memset(&c->stats, 0, sizeof(c->stats));
        c->stats.ms_total = elapsed_ms(c, EV_START, EV_FINAL);
        c->stats.n_reads = c->n; c->stats.read_bases = c->read_bases;
        if (hs.err) return check_device_err(c, hs.err);
        return HIMUT_OK;
    });
}

int himut_ref_tricounts(himut_ctx* c, int64_t out[64]) {
    if (!c || !out) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int {
        if (c->reflen <= 0) return fail(c, HIMUT_ERR_ARG, "himut_set_reference has not been called");
        HCHECK(hipSetDevice(c->device));
        c->d_tmp2.reserve(64 * 8 + 256);
        unsigned long long* d = c->d_tmp2.as<unsigned long long>();
        HCHECK(hipMemsetAsync(d, 0, 64 * 8, c->stream));
        HCHECK(hipEventRecord(c->ev[EV_START], c->stream));
        launch_fasta_tricounts(c->d_refseq.as<uint8_t>(), c->reflen, 0, d, c->stream);
        HCHECK(hipEventRecord(c->ev[EV_FINAL], c->stream));
        unsigned long long h[64];
        HCHECK(hipMemcpyAsync(h, d, 64 * 8, hipMemcpyDeviceToHost, c->stream));
        HCHECK(hipStreamSynchronize(c->stream));
        for (int k = 0; k < 64; k++) out[k] = (int64_t)h[k];
        c->stats.ms_total = elapsed_ms(c, EV_START, EV_FINAL);      // himut_get_stats: the kernel alone
        return HIMUT_OK;
    });
}

int himut_fasta_tricounts(himut_ctx* c, const uint8_t* body, int64_t n, int64_t out[64]) {
    if (!c || !out || n < 0 || (n && !body)) return HIMUT_ERR_ARG;
    if (!claim_pinned(c, false)) return fail(c, HIMUT_ERR_ARG, "an ingest is open: the two pinned windows belong to the process");
    struct Release { himut_ctx* c; ~Release() { release_pinned(c); } } rel{c};   // (only what this call claimed)
    return guarded(c, [&]() -> int {
        HCHECK(hipSetDevice(c->device));
        hipStream_t st = c->stream, cp = c->side;
        const int64_t W = c->dbg_fasta_window > 0 ? c->dbg_fasta_window : FASTA_WINDOW;
        const size_t cap = (size_t)std::min<int64_t>(W, std::max<int64_t>(n, 1));
        void* pinned[2];
        size_pinned(c, cap, hipHostMallocNonCoherent | hipHostMallocPortable, pinned);
        c->d_tmp2.reserve(64 * 8 + 256);
        unsigned long long* d = c->d_tmp2.as<unsigned long long>();
        HCHECK(hipMemsetAsync(d, 0, 64 * 8, st));
        HCHECK(hipStreamSynchronize(st));
        // window k: host memcpy into pinned[k & 1] (once the copy of window k - 2 is out of it), pinned -> HBM on the
        // copy stream (once the count of window k - 2 is done with the staging buffer), count on the compute stream;
        // the count of window k runs while the host fills window k + 1
        bool used[2] = {false, false};
        int64_t k = 0;
        for (int64_t s = 0; s < n; s += W, k++) {
            const int slot = (int)(k & 1);
            const int64_t e = std::min(n, s + W), nb = e - s;
            uint32_t tail = 0;                      // the first two letters behind the window (whitespace skipped)
            for (int64_t j = e; j < n && (tail & 3) < 2; j++) {
                const uint8_t b = body[j];
                if (b == '\n' || b == '\r' || b == '\t' || b == ' ') continue;
                const int code = b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 4;
                tail = follow_push(tail, code);
            }
            if (used[slot]) HCHECK(hipEventSynchronize(c->stage_copied[slot]));
            memcpy(pinned[slot], body + s, (size_t)nb);
            if (used[slot]) HCHECK(hipStreamWaitEvent(cp, c->stage_parsed[slot], 0));
            HCHECK(hipMemcpyAsync(c->d_stage[slot].p, pinned[slot], (size_t)nb, hipMemcpyHostToDevice, cp));
            HCHECK(hipEventRecord(c->stage_copied[slot], cp));
            HCHECK(hipStreamWaitEvent(st, c->stage_copied[slot], 0));
            launch_fasta_tricounts(c->d_stage[slot].as<uint8_t>(), nb, tail, d, st);
            HCHECK(hipEventRecord(c->stage_parsed[slot], st));
            used[slot] = true;
        }
        unsigned long long h[64];
        HCHECK(hipMemcpyAsync(h, d, 64 * 8, hipMemcpyDeviceToHost, st));
        HCHECK(hipStreamSynchronize(st));
        HCHECK(hipStreamSynchronize(cp));
        for (int b = 0; b < 64; b++) out[b] = (int64_t)h[b];
        return HIMUT_OK;
    });
}

int himut_debug_fasta_window(himut_ctx* c, int64_t window_bytes) {
    if (!c || window_bytes < 0) return HIMUT_ERR_ARG;
    c->dbg_fasta_window = window_bytes;
    return HIMUT_OK;
}

int himut_sbs96_counts(himut_ctx* c, const int32_t* pos0, const uint8_t* ref, const uint8_t* alt, int64_t n, int64_t out[99]) {
    return sbs_counts<1>(c, pos0, ref, alt, n, out);
}

int himut_sbs1536_counts(himut_ctx* c, const int32_t* pos0, const uint8_t* ref, const uint8_t* alt, int64_t n, int64_t out[1539]) {
    return sbs_counts<2>(c, pos0, ref, alt, n, out);
}

}  // extern "C"
