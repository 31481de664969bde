// libhimut_hip.so: the haplotag run (himut_run_haplotag, himut_get_haplotag) over the kernel of himut_haplotag.h.  The cs
// decode in front of it is the read pass every pipeline starts with (run_parse_stage, himut_front.hip), under a
// parameter block of the run's own; the scalars are its own too, as the support run's are.
#include <hip/hip_runtime.h>

#include "himut_ctx.h"
#include "himut_haplotag.h"

using namespace himut;

namespace {

// the rules of the hetSNP arrays and the parameters; the message names the one that broke (and is built only then)
int check_haplotag_args(himut_ctx* c, const int32_t* pos1, const uint8_t* ref, const uint8_t* alt, const uint8_t* bit, const int32_t* set,
                        int64_t n, int32_t n_sets, const himut_haplotag_params* p) {
    auto broke = [&](const char* rule, int64_t k = -1) {
        return fail(c, HIMUT_ERR_ARG, std::string("himut_run_haplotag: ") + rule + (k < 0 ? "" : " (hetSNP " + std::to_string(k) + ")"));
    };
    if (!p) return broke("params is null");
    if (n < 0 || n > INT32_MAX) return broke("n must lie in 0..2^31-1");
    if (n_sets < 0) return broke("n_sets is negative");
    if (n && (!pos1 || !ref || !alt || !bit || !set)) return broke("a hetSNP array is null while n > 0");
    if (p->min_snps < 1) return broke("min_snps must be at least 1");
    if (p->min_agree_permille < 501 || p->min_agree_permille > 1000) return broke("min_agree_permille must lie in 501..1000");
    auto acgt = [](uint8_t b) { return b == 'A' || b == 'C' || b == 'G' || b == 'T'; };
    for (int64_t k = 0; k < n; k++) {
        if (pos1[k] < 1) return broke("pos1 must be 1-based", k);
        if (k && pos1[k] <= pos1[k - 1]) return broke("pos1 must be strictly ascending", k);
        if (!acgt(ref[k]) || !acgt(alt[k])) return broke("ref and alt must be upper-case letters of ACGT", k);
        if (ref[k] == alt[k]) return broke("ref and alt must differ", k);
        if (bit[k] > 1) return broke("bit must be 0 or 1", k);
        if (set[k] < 0 || set[k] >= n_sets) return broke("set must lie in 0..n_sets-1", k);
    }
    return HIMUT_OK;
}

}  // namespace

extern "C" {

int himut_run_haplotag(himut_ctx* c, const int32_t* pos1, const uint8_t* ref, const uint8_t* alt, const uint8_t* bit, const int32_t* set,
                       int64_t n, int32_t n_sets, const himut_haplotag_params* p) {
    if (!c) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int {
        if (int rc = check_haplotag_args(c, pos1, ref, alt, bit, set, n, n_sets, p)) return rc;
        if (int rc = check_run_inputs(c, NEED_READS)) return rc;
        HCHECK(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        himut_ctx::Haplotag& H = c->haplotag;
        memset(&c->stats, 0, sizeof(c->stats));
        std::vector<himut_haplotag_row> rows((size_t)c->n);
        std::vector<himut_haplotag_snp> snps((size_t)n);

        alloc_derived(c);
        const size_t row_bytes = (size_t)c->n * sizeof(himut_haplotag_row), snp_bytes = (size_t)n * sizeof(himut_haplotag_snp);
        H.d_rows.reserve(row_bytes + 256);
        H.d_snps.reserve(snp_bytes + 256);
        H.d_sc.reserve(sizeof(Scalars));
        upload(H.d_pos, pos1, (size_t)n, st); upload(H.d_ref, ref, (size_t)n, st); upload(H.d_alt, alt, (size_t)n, st);
        upload(H.d_bit, bit, (size_t)n, st); upload(H.d_set, set, (size_t)n, st);
        Scalars* sc = H.d_sc.as<Scalars>();        // (not the context's: the other runs keep theirs as they left them)
        Scalars hs;
        memset(&hs, 0, sizeof(hs));

        HCHECK(hipEventRecord(c->ev[EV_START], st));
        HCHECK(hipMemsetAsync(sc, 0, sizeof(Scalars), st));
        HCHECK(hipMemsetAsync(H.d_snps.p, 0, snp_bytes + 256, st));
        // the decode marks nothing (no bitmap) and flags every read's identity as passing: query-length limits open, identity -1
        const Params P = open_gate_params(c, p->min_mapq);
        HaplotagArgs A;
        A.R = make_reads(c); A.D = make_derived(c);
        A.pos1 = H.d_pos.as<int32_t>(); A.ref = H.d_ref.as<uint8_t>(); A.alt = H.d_alt.as<uint8_t>();
        A.bit = H.d_bit.as<uint8_t>(); A.set = H.d_set.as<int32_t>(); A.nsnps = n;
        A.min_mapq = p->min_mapq; A.min_bq = p->min_bq; A.min_snps = p->min_snps; A.min_agree_permille = p->min_agree_permille;
        A.rows = H.d_rows.as<himut_haplotag_row>(); A.snps = H.d_snps.as<uint32_t>();
        A.log = sc->log; A.err = &sc->err;
        if (c->n > 0) {
            run_parse_stage(c, A.R, A.D, sc, &P);
            hipLaunchKernelGGL(k_haplotag, dim3(blocks_for(c->n, 16)), dim3(256), 0, st, A);
        } else {
            stage_event(c, EV_PARSE, 2, st);
        }
        HCHECK(hipEventRecord(c->ev[EV_FINAL], st));
        HCHECK(hipMemcpyAsync(&hs, sc, sizeof(Scalars), hipMemcpyDeviceToHost, st));
        if (c->n) HCHECK(hipMemcpyAsync(rows.data(), H.d_rows.p, row_bytes, hipMemcpyDeviceToHost, st));
        if (n) HCHECK(hipMemcpyAsync(snps.data(), H.d_snps.p, snp_bytes, hipMemcpyDeviceToHost, st));
        HCHECK(hipStreamSynchronize(st));
        if (hs.err) return check_device_err(c, hs.err);
        H.h_rows.swap(rows);
        H.h_snps.swap(snps);
        for (int k = 0; k < 13; k++) H.log[k] = (int64_t)hs.log[k];
        c->stats.ms_total = elapsed_ms(c, EV_START, EV_FINAL);
        if (c->timing >= 2) {       // the clearing and the decode; the rows, the tallies and the counters
            c->stats.ms_parse = elapsed_ms(c, EV_START, EV_PARSE);
            c->stats.ms_eval = elapsed_ms(c, EV_PARSE, EV_FINAL);
        }
        c->stats.n_reads = c->n; c->stats.read_bases = c->read_bases; c->stats.n_records = c->n; c->stats.positions = n;
        return HIMUT_OK;
    });
}

int himut_get_haplotag(himut_ctx* c, const himut_haplotag_row** rows, int64_t* n_rows, const himut_haplotag_snp** snps, int64_t* n_snps,
                       int64_t log[13]) {
    if (!c) return HIMUT_ERR_ARG;
    const himut_ctx::Haplotag& H = c->haplotag;
    if (rows) *rows = H.h_rows.data();
    if (n_rows) *n_rows = (int64_t)H.h_rows.size();
    if (snps) *snps = H.h_snps.data();
    if (n_snps) *n_snps = (int64_t)H.h_snps.size();
    if (log) std::copy(H.log, H.log + 13, log);
    return HIMUT_OK;
}

}  // extern "C"
