// libhimut_hip.so: the device-side BAM ingest (himut_ingest_*) over the kernels of himut_ingest.h, and the read
// batch back on the host (himut_download_reads).
#include <hip/hip_runtime.h>

#include <string.h>  // rocprim's texture iterator needs the host memset declared first
#include <rocprim/rocprim.hpp>

#include <chrono>
#include <cstdlib>

#include "himut_ctx.h"
#include "himut_ingest.h"

using namespace himut;

namespace {

// First sizes of the contig's arrays from what CCS records look like (two thirds of a record are qualities); the arrays
// grow if a window needs more.
void ingest_size_arrays(himut_ctx* c, hipStream_t st) {
    const size_t B = c->ingest.bound;
    c->d_bq.reserve(B * 7 / 10 + (1 << 20));
    c->d_seq.reserve(B * 7 / 20 + (1 << 20));
    c->d_cs.reserve(B / 16 + (1 << 20));
    const size_t nr0 = B / 4000 + 4096;
    c->d_tstart.reserve(nr0 * 4 + 256); c->d_tend.reserve(nr0 * 4 + 256); c->d_qstart.reserve(nr0 * 4 + 256); c->d_qlen.reserve(nr0 * 4 + 256);
    c->d_qid.reserve(nr0 * 4 + 256); c->d_mapq.reserve(nr0 + 256); c->ingest.d_tp.reserve(nr0 + 256); c->d_flag.reserve(nr0 * 2 + 256);
    c->d_qoff.reserve(nr0 * 8 + 256); c->d_csoff.reserve((nr0 + 1) * 8 + 256);
    HCHECK(hipMemsetAsync(c->d_csoff.p, 0, 8, st));
    if (c->ingest.derive_on) {
        // the CIGAR words of a CCS record: a few hundred bytes; like the others the arrays grow if a window needs more
        c->ingest.d_cig.reserve(B / 32 + (1 << 20));
        c->ingest.d_cigoff.reserve((nr0 + 1) * 8 + 256);
        HCHECK(hipMemsetAsync(c->ingest.d_cigoff.p, 0, 8, st));
    }
    c->ingest.sized = true;
}

// The post-pass of an ingest that derives the cs text: the CIGAR side array, SEQ and the resident reference into d_cs /
// d_csoff, exactly sized.  Returns the bytes of text; the refused records are counted in derive_res[1].
int64_t derive_cs_text(himut_ctx* c, int64_t n, hipStream_t st) {
    himut_ctx::Ingest& I = c->ingest;
    I.d_cslen.reserve((size_t)(n + 1) * 8 + 256);
    I.d_csbad.reserve((size_t)n + 256);
    I.d_dstate.reserve(256);
    HCHECK(hipMemsetAsync(I.d_dstate.p, 0, 8, st));
    HCHECK(hipMemsetAsync((uint8_t*)I.d_cslen.p + (size_t)n * 8, 0, 8, st));
    size_t scan_b = 0;
    HCHECK(rocprim::exclusive_scan(nullptr, scan_b, I.d_cslen.as<unsigned long long>(), c->d_csoff.as<unsigned long long>(), 0ull, (size_t)n + 1,
                                   rocprim::plus<unsigned long long>(), st));
    c->d_tmp.reserve(scan_b + 256);
    CsDerive A;
    A.n = n; A.tstart = c->d_tstart.as<int32_t>(); A.qlen = c->d_qlen.as<int32_t>(); A.qoff = c->d_qoff.as<int64_t>();
    A.cig_off = I.d_cigoff.as<int64_t>(); A.seq = c->d_seq.as<uint8_t>(); A.cig = I.d_cig.as<uint8_t>();
    A.ref = c->d_refseq.as<uint8_t>(); A.reflen = c->reflen;
    A.len = I.d_cslen.as<unsigned long long>(); A.bad = I.d_csbad.as<uint8_t>(); A.n_bad = I.d_dstate.as<unsigned long long>();
    A.cs_off = c->d_csoff.as<int64_t>(); A.cs = nullptr;
    HCHECK(hipEventRecord(c->ev[EV_START], st));
    if (n) hipLaunchKernelGGL(k_cs_measure, dim3(blocks_for(n, 4)), dim3(256), 0, st, A);
    HCHECK(rocprim::exclusive_scan(c->d_tmp.p, scan_b, I.d_cslen.as<unsigned long long>(), c->d_csoff.as<unsigned long long>(), 0ull, (size_t)n + 1,
                                   rocprim::plus<unsigned long long>(), st));
    HCHECK(hipEventRecord(c->ev[EV_PARSE], st));
    HCHECK(hipStreamSynchronize(st));
    int64_t total = 0;
    unsigned long long n_bad = 0;
    HCHECK(hipMemcpy(&total, (const uint8_t*)c->d_csoff.p + (size_t)n * 8, 8, hipMemcpyDeviceToHost));
    HCHECK(hipMemcpy(&n_bad, I.d_dstate.p, 8, hipMemcpyDeviceToHost));
    // the kernels behind read 1 KB of cs text past the end: the array carries that slack
    c->d_cs.reserve((size_t)total + 2048 + 256);
    A.cs = c->d_cs.as<uint8_t>();
    HCHECK(hipEventRecord(c->ev[EV_EMIT], st));
    if (n) hipLaunchKernelGGL(k_cs_emit, dim3(blocks_for(n, 4)), dim3(256), 0, st, A);
    HCHECK(hipEventRecord(c->ev[EV_FINAL], st));
    HCHECK(hipStreamSynchronize(st));
    I.derive_res[0] = n - (int64_t)n_bad; I.derive_res[1] = (int64_t)n_bad; I.derive_res[2] = total;
    // device time of the two halves; the host's look at the total and the allocation of d_cs lie between them
    I.derive_ms = elapsed_ms(c, EV_START, EV_PARSE) + elapsed_ms(c, EV_EMIT, EV_FINAL);
    if (getenv("HIMUT_INGEST_PROFILE"))
        fprintf(stderr, "ingest: cs text of %lld reads derived in %.3f ms (measure + scan %.3f, emit %.3f; %lld bytes, %llu records refused)\n",
                (long long)n, I.derive_ms, elapsed_ms(c, EV_START, EV_PARSE), elapsed_ms(c, EV_EMIT, EV_FINAL), (long long)total, n_bad);
    I.d_cig.release(); I.d_cigoff.release(); I.d_cslen.release(); I.d_csbad.release();
    return total;
}

}  // namespace

extern "C" {

int himut_ingest_begin(himut_ctx* c, int64_t inflated_bound, int64_t window_bytes) {
    if (!c || inflated_bound < 0 || window_bytes < (1 << 16)) return fail(c, HIMUT_ERR_ARG, "bad ingest arguments");
    if (c->ingest.derive && c->reflen <= 0) return fail(c, HIMUT_ERR_ARG, "deriving the cs text needs himut_set_reference");
    return guarded(c, [&]() -> int {
        HCHECK(hipSetDevice(c->device));
        HCHECK(hipStreamSynchronize(c->stream));
        HCHECK(hipStreamSynchronize(c->side));
        const size_t W = (size_t)window_bytes;
        // one ingest at a time: the two pinned windows belong to the process
        if (!claim_pinned(c, true))
            return fail(c, HIMUT_ERR_ARG, "another context's ingest is open: the two pinned windows belong to the process");
        const auto t_pin = std::chrono::steady_clock::now();
        // cacheable pages: the inflate reads its own output back (LZ77 matches)
        const unsigned fl = getenv("HIMUT_PINNED_COHERENT") ? hipHostMallocDefault : (hipHostMallocNonCoherent | hipHostMallocPortable);
        if (size_pinned(c, W, fl, c->ingest.pinned) && getenv("HIMUT_INGEST_PROFILE"))
            fprintf(stderr, "ingest: pinned windows 2 x %zu MB in %.1f ms\n", (W + 4096) >> 20,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_pin).count());
        c->ingest.window = W;
        for (int k = 0; k < 2; k++) c->ingest.used[k] = false;
        // the contig's arrays are sized when the first window arrives (himut_ingest_window): by then the host's pool
        // is inflating the second window, and gigabytes of hipMalloc are off the path
        c->ingest.bound = (size_t)inflated_bound;
        c->ingest.sized = false;
        c->ingest.d_istate.reserve(sizeof(IngestState));
        IngestState z;
        memset(&z, 0, sizeof(z));
        z.last_pos = -0x7fffffff - 1;
        HCHECK(hipMemcpy(c->ingest.d_istate.p, &z, sizeof(z), hipMemcpyHostToDevice));
        c->ingest.reads = c->ingest.bases = c->ingest.cs = 0;
        c->ingest.derive_on = c->ingest.derive != 0;
        for (int k = 0; k < 3; k++) c->ingest.derive_res[k] = 0;
        c->ingest.derive_ms = 0;
        c->ingest.open = true;
        c->have_reads = false;
        forget_reads(c);
        return HIMUT_OK;
    });
}

void* himut_ingest_buffer(himut_ctx* c, int slot) { return (c && (slot == 0 || slot == 1)) ? c->ingest.pinned[slot] : nullptr; }

int himut_ingest_wait(himut_ctx* c, int slot) {
    if (!c || (slot != 0 && slot != 1)) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int {
        if (c->ingest.used[slot]) HCHECK(hipEventSynchronize(c->stage_copied[slot]));
        return HIMUT_OK;
    });
}

int himut_ingest_window(himut_ctx* c, int slot, int64_t start, int64_t nbytes, const uint32_t* rec_off, const int32_t* qid, int64_t n_rec,
                        int64_t padded_bases, int64_t tag_bytes) {
    if (!c || (slot != 0 && slot != 1) || n_rec < 0 || nbytes < 0 || start < 0 || (n_rec && (!rec_off || !qid)))
        return fail(c, HIMUT_ERR_ARG, "bad ingest window");
    if (!c->ingest.open) return fail(c, HIMUT_ERR_ARG, "himut_ingest_begin has not been called");
    if ((size_t)(start + nbytes) > c->ingest.window) return fail(c, HIMUT_ERR_ARG, "ingest window larger than the buffer");
    if (n_rec == 0) return HIMUT_OK;
    return guarded(c, [&]() -> int {
        HCHECK(hipSetDevice(c->device));
        hipStream_t st = c->stream, cp = c->side;
        if (!c->ingest.sized) {
            const auto t_sz = std::chrono::steady_clock::now();
            ingest_size_arrays(c, st);
            if (getenv("HIMUT_INGEST_PROFILE"))
                fprintf(stderr, "ingest: contig arrays sized in %.1f ms\n",
                        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_sz).count());
        }
        // room for this window's reads: exact for the per-read arrays and the bases, an upper bound for the cs text
        const int64_t nr = c->ingest.reads + n_rec, nb = c->ingest.bases + padded_bases, nc = c->ingest.cs + tag_bytes;
        const size_t ur = (size_t)c->ingest.reads;
        c->d_tstart.grow_keep((size_t)nr * 4 + 256, ur * 4); c->d_tend.grow_keep((size_t)nr * 4 + 256, ur * 4);
        c->d_qstart.grow_keep((size_t)nr * 4 + 256, ur * 4); c->d_qlen.grow_keep((size_t)nr * 4 + 256, ur * 4);
        c->d_qid.grow_keep((size_t)nr * 4 + 256, ur * 4); c->d_mapq.grow_keep((size_t)nr + 256, ur); c->ingest.d_tp.grow_keep((size_t)nr + 256, ur);
        c->d_flag.grow_keep((size_t)nr * 2 + 256, ur * 2); c->d_qoff.grow_keep((size_t)nr * 8 + 256, ur * 8);
        c->d_csoff.grow_keep((size_t)(nr + 1) * 8 + 256, (ur + 1) * 8);
        c->d_bq.grow_keep((size_t)nb + 256, (size_t)c->ingest.bases); c->d_seq.grow_keep((size_t)nb / 2 + 256, (size_t)c->ingest.bases / 2);
        const bool derive = c->ingest.derive_on;
        // a deriving ingest keeps the CIGAR words (tag_bytes counts them) in a side array; d_cs is sized by the post-pass
        if (derive) {
            c->ingest.d_cig.grow_keep((size_t)nc + 256, (size_t)c->ingest.cs);
            c->ingest.d_cigoff.grow_keep((size_t)(nr + 1) * 8 + 256, (ur + 1) * 8);
        } else {
            c->d_cs.grow_keep((size_t)nc + 2048 + 256, (size_t)c->ingest.cs);
        }
        c->ingest.d_recoff[slot].reserve((size_t)n_rec * 4 + 256); c->ingest.d_qidin[slot].reserve((size_t)n_rec * 4 + 256);
        c->ingest.d_desc.reserve((size_t)n_rec * sizeof(RecDesc) + 256);
        c->ingest.d_sizes.reserve((size_t)n_rec * 8 + 256); c->ingest.d_offs.reserve((size_t)n_rec * 8 + 256);
        size_t scan_b = 0;
        HCHECK(rocprim::exclusive_scan(nullptr, scan_b, c->ingest.d_sizes.as<uint2>(), c->ingest.d_offs.as<uint2>(), make_uint2(0u, 0u), (size_t)n_rec, PlusU2(), st));
        c->d_tmp.reserve(scan_b + 256);
        // copy stream: the window's bytes (pinned -> HBM) once the parse of the window that used this staging buffer is over
        if (c->ingest.used[slot]) HCHECK(hipStreamWaitEvent(cp, c->stage_parsed[slot], 0));
        HCHECK(hipMemcpyAsync(c->d_stage[slot].p, (const uint8_t*)c->ingest.pinned[slot] + start, (size_t)nbytes, hipMemcpyHostToDevice, cp));
        HCHECK(hipEventRecord(c->stage_copied[slot], cp));
        c->ingest.used[slot] = true;
        // compute stream: record list, decode, offsets, scatter
        HCHECK(hipMemcpyAsync(c->ingest.d_recoff[slot].p, rec_off, (size_t)n_rec * 4, hipMemcpyHostToDevice, st));
        HCHECK(hipMemcpyAsync(c->ingest.d_qidin[slot].p, qid, (size_t)n_rec * 4, hipMemcpyHostToDevice, st));
        HCHECK(hipStreamWaitEvent(st, c->stage_copied[slot], 0));
        const uint8_t* win = c->d_stage[slot].as<uint8_t>();
        hipLaunchKernelGGL(k_bam_decode, dim3(blocks_for(n_rec, 256)), dim3(256), 0, st, win, nbytes, c->ingest.d_recoff[slot].as<uint32_t>(), n_rec,
                           c->ingest.d_desc.as<RecDesc>(), c->ingest.d_sizes.as<uint2>(), derive ? 1 : 0);
        HCHECK(rocprim::exclusive_scan(c->d_tmp.p, scan_b, c->ingest.d_sizes.as<uint2>(), c->ingest.d_offs.as<uint2>(), make_uint2(0u, 0u), (size_t)n_rec, PlusU2(), st));
        IngestOut O;
        O.tstart = c->d_tstart.as<int32_t>(); O.tend = c->d_tend.as<int32_t>(); O.qstart = c->d_qstart.as<int32_t>(); O.qlen = c->d_qlen.as<int32_t>();
        O.qid = c->d_qid.as<int32_t>(); O.mapq = c->d_mapq.as<uint8_t>(); O.tp = c->ingest.d_tp.as<uint8_t>(); O.flag = c->d_flag.as<uint16_t>();
        O.qoff = c->d_qoff.as<int64_t>(); O.cs_off = derive ? c->ingest.d_cigoff.as<int64_t>() : c->d_csoff.as<int64_t>();
        O.seq = c->d_seq.as<uint8_t>(); O.bq = c->d_bq.as<uint8_t>(); O.cs = derive ? c->ingest.d_cig.as<uint8_t>() : c->d_cs.as<uint8_t>();
        O.cap_reads = nr; O.cap_bases = nb; O.cap_cs = nc;
        hipLaunchKernelGGL(k_bam_scatter, dim3(blocks_for(n_rec, 4)), dim3(256), 0, st, win, c->ingest.d_desc.as<RecDesc>(), c->ingest.d_offs.as<uint2>(),
                           c->ingest.d_qidin[slot].as<int32_t>(), n_rec, O, c->ingest.d_istate.as<IngestState>(), derive ? 1 : 0);
        hipLaunchKernelGGL(k_bam_advance, dim3(1), dim3(64), 0, st, c->ingest.d_desc.as<RecDesc>(), c->ingest.d_sizes.as<uint2>(), c->ingest.d_offs.as<uint2>(), n_rec,
                           c->ingest.d_istate.as<IngestState>(), O.cs_off, nr);
        HCHECK(hipEventRecord(c->stage_parsed[slot], st));
        c->ingest.reads = nr; c->ingest.bases = nb; c->ingest.cs = nc;
        return HIMUT_OK;
    });
}

int himut_ingest_end(himut_ctx* c, int unique_qnames, himut_ingest_result* out) {
    if (!c || !out) return HIMUT_ERR_ARG;
    if (!c->ingest.open) return fail(c, HIMUT_ERR_ARG, "himut_ingest_begin has not been called");
    return guarded(c, [&]() -> int {
        HCHECK(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        if (!c->ingest.sized) { c->ingest.bound = 0; ingest_size_arrays(c, st); }       // a contig without records
        HCHECK(hipStreamSynchronize(c->side));
        HCHECK(hipStreamSynchronize(st));
        c->ingest.open = false;
        release_pinned(c);
        IngestState S;
        HCHECK(hipMemcpy(&S, c->ingest.d_istate.p, sizeof(S), hipMemcpyDeviceToHost));
        memset(out, 0, sizeof(*out));
        out->n_reads = (int64_t)S.n_reads; out->bases_padded = (int64_t)S.bases_padded; out->cs_bytes = (int64_t)S.cs_n;
        out->read_bases = (int64_t)S.read_bases; out->n_missing_cs = (int64_t)S.n_missing_cs; out->n_unsorted = (int64_t)S.n_unsorted;
        out->n_malformed = (int64_t)S.n_bad;
        if (S.overflow) return fail(c, HIMUT_ERR_NOMEM, "ingest: a window needed more room than the host announced");
        if (S.n_bad) return fail(c, HIMUT_ERR_ARG, "malformed BAM record");
        const int64_t n = (int64_t)S.n_reads;
        const bool derive = c->ingest.derive_on;
        if (derive) {
            // S.cs_n counted CIGAR bytes: the text and its offsets come from the post-pass, after which nothing behind
            // this point sees a difference from a file with tags
            S.cs_n = (unsigned long long)derive_cs_text(c, n, st);
            S.any_longcs = 0;
            out->cs_bytes = (int64_t)S.cs_n;
        }
        c->n = n; c->cs_bytes = (int64_t)S.cs_n; c->bq_bytes = (int64_t)S.bases_padded; c->seq_bytes = (int64_t)S.bases_padded / 2;
        c->read_bases = (int64_t)S.read_bases;
        c->unique_qnames = unique_qnames != 0;
        c->any_longcs = S.any_longcs != 0;
        c->h_tstart.resize((size_t)n); c->h_tend.resize((size_t)n); c->h_prefmax.resize((size_t)n);
        if (n) {
            HCHECK(hipMemcpy(c->h_tstart.data(), c->d_tstart.p, (size_t)n * 4, hipMemcpyDeviceToHost));
            HCHECK(hipMemcpy(c->h_tend.data(), c->d_tend.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        }
        int32_t run = INT32_MIN;
        for (int64_t i = 0; i < n; i++) { run = std::max(run, c->h_tend[(size_t)i]); c->h_prefmax[(size_t)i] = run; }
        upload(c->d_prefmax, c->h_prefmax, st);
        // the kernels read whole 16 / 32-byte windows and 1 KB of cs text past the end: the arrays carry that slack
        if (!derive) c->d_cs.grow_keep((size_t)S.cs_n + 2048 + 256, (size_t)S.cs_n);
        HCHECK(hipStreamSynchronize(st));
        c->have_reads = S.n_unsorted == 0 && S.n_missing_cs == 0 && c->ingest.derive_res[1] == 0;
        forget_reads(c);
        return HIMUT_OK;
    });
}

int himut_ingest_derive_cs(himut_ctx* c, int mode) {
    if (!c) return HIMUT_ERR_ARG;
    if (mode != 0 && mode != 1) return fail(c, HIMUT_ERR_ARG, "himut_ingest_derive_cs: mode is 0 or 1");
    if (mode == 1 && c->reflen <= 0) return fail(c, HIMUT_ERR_ARG, "deriving the cs text needs himut_set_reference");
    c->ingest.derive = mode;
    return HIMUT_OK;
}

int himut_ingest_derive_result(himut_ctx* c, int64_t out[4]) {
    if (!c || !out) return HIMUT_ERR_ARG;
    for (int k = 0; k < 3; k++) out[k] = c->ingest.derive_res[k];
    out[3] = (int64_t)(c->ingest.derive_ms + 0.5);
    return HIMUT_OK;
}

int himut_ingest_read_meta(himut_ctx* c, int32_t* tstart, int32_t* tend, int32_t* qlen, uint8_t* mapq, uint8_t* tp) {
    if (!c) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int {
        HCHECK(hipSetDevice(c->device));
        const size_t n = (size_t)c->n;
        if (!n) return HIMUT_OK;
        if (tstart) HCHECK(hipMemcpy(tstart, c->d_tstart.p, n * 4, hipMemcpyDeviceToHost));
        if (tend) HCHECK(hipMemcpy(tend, c->d_tend.p, n * 4, hipMemcpyDeviceToHost));
        if (qlen) HCHECK(hipMemcpy(qlen, c->d_qlen.p, n * 4, hipMemcpyDeviceToHost));
        if (mapq) HCHECK(hipMemcpy(mapq, c->d_mapq.p, n, hipMemcpyDeviceToHost));
        if (tp) HCHECK(hipMemcpy(tp, c->ingest.d_tp.p, n, hipMemcpyDeviceToHost));
        return HIMUT_OK;
    });
}

// The read batch as it sits in HBM, back on the host (tests: the device-parsed batch against the host-parsed one).
int himut_download_reads(himut_ctx* c, himut_read_batch* b, uint8_t* tp) {
    if (!c || !b) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int {
        HCHECK(hipSetDevice(c->device));
        const size_t n = (size_t)c->n;
        if (b->n_reads < c->n || b->seq_bytes < c->seq_bytes || b->bq_bytes < c->bq_bytes || b->cs_bytes < c->cs_bytes)
            return fail(c, HIMUT_ERR_ARG, "destination batch too small");
        auto down = [&](const void* dst, const DevBuf& src, size_t bytes) { if (bytes) HCHECK(hipMemcpy(const_cast<void*>(dst), src.p, bytes, hipMemcpyDeviceToHost)); };
        down(b->tstart, c->d_tstart, n * 4); down(b->tend, c->d_tend, n * 4); down(b->qstart, c->d_qstart, n * 4); down(b->qlen, c->d_qlen, n * 4);
        down(b->mapq, c->d_mapq, n); down(b->flag, c->d_flag, n * 2); down(b->qid, c->d_qid, n * 4); down(b->qoff, c->d_qoff, n * 8);
        down(b->cs_off, c->d_csoff, (n + 1) * 8);
        down(b->seq, c->d_seq, (size_t)c->seq_bytes); down(b->bq, c->d_bq, (size_t)c->bq_bytes); down(b->cs, c->d_cs, (size_t)c->cs_bytes);
        if (tp) down(tp, c->ingest.d_tp, n);
        b->n_reads = c->n; b->seq_bytes = c->seq_bytes; b->bq_bytes = c->bq_bytes; b->cs_bytes = c->cs_bytes;
        return HIMUT_OK;
    });
}

}  // extern "C"
