// libhimut_hip.so: the duplex run (himut_run_duplex, himut_get_duplex) over the kernels of himut_duplex.h.  The run is the
// sites run's pass (sites_front, sites_back: himut_sites.hip) on buffers of its own, with the site list made on the
// device between the two steps: behind the decode the reads' verdicts, the events of the pairs in play (a counted key
// list -- count_keys, sort_with_tmp: himut_ctx.h, as the dbs run's proposals), the denominator, the keys' sort and
// run-length encoding, and the per-candidate tallies; behind the pass one kernel joins the site records and the tallies.
// Two capacities are kept from run to run (the keys, the column store); the repeat is run_repeating.
#include <hip/hip_runtime.h>

#include <string.h>  // rocprim's texture iterator needs the host memset declared first
#include <rocprim/rocprim.hpp>

#include "himut_ctx.h"
#include "himut_duplex.h"

using namespace himut;

namespace {

constexpr int KEY_BITS = 36;     // duplex_key: a 32-bit position and four bits of alleles

// mate[] under the contract's rules; the message names the read that breaks one
int check_mate(himut_ctx* c, const int32_t* mate, int64_t n_mate, const himut_duplex_params* p) {
    auto broke = [&](const std::string& what) { return fail(c, HIMUT_ERR_ARG, "himut_run_duplex: " + what); };
    if (!p) return broke("params is null");
    for (int32_t w : p->reserved) if (w != 0) return broke("a reserved word of params is not zero");
    if (n_mate != c->n) return broke("n_mate is " + std::to_string(n_mate) + ", the context holds " + std::to_string(c->n) + " reads");
    if (n_mate > 0 && !mate) return broke("mate is null while n_mate > 0");
    for (int64_t i = 0; i < n_mate; i++) {
        const int64_t m = mate[i];
        if (m == -1) continue;
        if (m < -1 || m >= n_mate) return broke("mate[" + std::to_string(i) + "] = " + std::to_string(m) + " lies outside -1.." + std::to_string(n_mate - 1));
        if (m == i) return broke("mate[" + std::to_string(i) + "] is the read itself");
        if (mate[m] != i) return broke("mate[" + std::to_string(i) + "] = " + std::to_string(m) + ", but mate[" + std::to_string(m) + "] = " + std::to_string(mate[m]));
    }
    return HIMUT_OK;
}

hipError_t sort_keys(himut_ctx* c, void* tmp, size_t& bytes, int64_t n) {
    himut_ctx::Duplex& D = c->duplex;
    return rocprim::radix_sort_keys(tmp, bytes, D.d_keys.as<uint64_t>(), D.d_keys2.as<uint64_t>(), (size_t)n, 0, KEY_BITS, c->stream);
}

// the sorted keys' runs: the distinct keys, their lengths (n_ds) and their number
hipError_t encode_keys(himut_ctx* c, void* tmp, size_t& bytes, int64_t n) {
    himut_ctx::Duplex& D = c->duplex;
    return rocprim::run_length_encode(tmp, bytes, D.d_keys2.as<uint64_t>(), (unsigned int)n, D.d_uniq.as<uint64_t>(), D.d_nds.as<uint32_t>(),
                                      D.d_sc.as<unsigned long long>() + DX_W_NCAND, c->stream);
}

void reserve_for_keys(himut_ctx* c, int64_t cap) {
    himut_ctx::Duplex& D = c->duplex;
    D.d_keys.reserve((size_t)cap * 8 + 256);
    D.d_keys2.reserve((size_t)cap * 8 + 256);
    D.d_uniq.reserve((size_t)cap * 8 + 256);
    D.d_nds.reserve((size_t)cap * 4 + 256);
    if (cap > 0) {
        sort_with_tmp(D.d_sorttmp, false, [&](void* tmp, size_t& bytes) { return sort_keys(c, tmp, bytes, cap); });
        sort_with_tmp(D.d_rletmp, false, [&](void* tmp, size_t& bytes) { return encode_keys(c, tmp, bytes, cap); });
    }
}

// what depends on the number of candidates: the sites pass's arrays and records, the tallies, the run's records
void reserve_for_candidates(himut_ctx* c, int64_t ncand) {
    himut_ctx::Duplex& D = c->duplex;
    const size_t n1 = (size_t)ncand + 1;
    D.sites.d_pos.reserve(n1 * 4 + 256);
    D.sites.d_code.reserve(n1 + 256);
    D.sites.d_recs.reserve(n1 * sizeof(himut_site_record));
    D.d_tally.reserve(n1 * 8);
    D.d_recs.reserve(n1 * sizeof(himut_duplex_record));
}

// the stages of the run: the decode, the pair kernels (with the host's waits for their counts), the column index, the
// candidates' evaluation, the front's tail
const StageSpan DUPLEX_STAGES[] = {{&himut_run_stats::ms_parse, EV_START, EV_PARSE}, {&himut_run_stats::ms_hap, EV_PARSE, EV_HAP},
                                   {&himut_run_stats::ms_index, EV_HAP, EV_INDEX}, {&himut_run_stats::ms_eval, EV_GATHER, EV_SWEEP},
                                   {&himut_run_stats::ms_finalize, EV_SWEEP, EV_FINAL}};

// One pass; mate[] is in D.d_mate.  kept: the key buffers and the column store keep the capacities of the previous duplex
// run; *overflow is set if the keys or the column slots did not fit (the caller runs again with exact sizes).
int duplex_once(himut_ctx* c, bool allow_spec, bool* overflow) {
    *overflow = false;
    himut_ctx::Duplex& D = c->duplex;
    begin_run(c, D.out);
    std::fill(D.ss, D.ss + 12, (int64_t)0);
    hipStream_t st = c->stream;

    std::vector<int32_t> sstart, spmax;
    sorted_regions(c->cstart, c->cend, &sstart, &spmax);
    int64_t positions = 0;
    for (size_t k = 0; k < c->cstart.size(); k++) positions += std::max<int64_t>(0, (int64_t)c->cend[k] - c->cstart[k]);
    upload(D.d_sstart, sstart, st); upload(D.d_spmax, spmax, st);
    HCHECK(hipStreamSynchronize(st));                    // (the two vectors are locals: their copies must be over before they go)
    D.d_verdict.reserve((size_t)c->n + 256);
    D.d_sc.reserve(DX_WORDS * 8);
    const bool spec_keys = allow_spec && D.cap_keys > 0 && c->n > 0;
    if (spec_keys) reserve_for_keys(c, D.cap_keys);

    // the decode's block: call's identity threshold (RF_IDENT_OK is one of the read filters) and closed query-length
    // limits, so no read passes the bitmap gate and the decode marks nothing
    Params PD = c->params;
    PD.p.phase = 0;
    PD.p.qlen_lower_limit = INT_MAX; PD.p.qlen_upper_limit = -1;
    SitesFront SF = sites_front(c, D.sites, PD, allow_spec);
    Scalars* sc = c->d_scalars.as<Scalars>();
    unsigned long long* dsc = D.d_sc.as<unsigned long long>();

    KeyCount K{0, 0, false};
    int64_t ncand = 0;
    if (c->n > 0) {
        const himut_params& p = c->params.p;
        HCHECK(hipMemsetAsync(dsc, 0, DX_WORDS * 8, st));
        DuplexReadArgs RA{};
        RA.R = make_reads(c); RA.meta = c->d_meta.as<ReadMeta>();
        RA.min_mapq = p.min_mapq; RA.min_qv = p.min_qv; RA.qlen_lower_limit = p.qlen_lower_limit; RA.qlen_upper_limit = p.qlen_upper_limit;
        RA.verdict = D.d_verdict.as<uint8_t>(); RA.w = dsc; RA.err = &sc->err;
        hipLaunchKernelGGL(k_duplex_reads, dim3(blocks_for(c->n, 4)), dim3(256), 0, st, RA);

        DuplexArgs A{};
        A.R = RA.R; A.D = make_derived(c); A.p = p;
        A.mate = D.d_mate.as<int32_t>(); A.verdict = RA.verdict;
        A.s_start = D.d_sstart.as<int32_t>(); A.s_pmaxend = D.d_spmax.as<int32_t>(); A.nregion = (int64_t)sstart.size();
        A.w = dsc; A.err = &sc->err;
        K = count_keys(c, spec_keys, D.cap_keys, dsc + DX_W_NKEYS,
                       [&](int64_t cap) {
                           HCHECK(hipMemsetAsync(dsc + DX_ONCE_WORDS, 0, (DX_WORDS - DX_ONCE_WORDS) * 8, st));
                           A.keys = D.d_keys.as<uint64_t>(); A.cap_keys = cap;
                           hipLaunchKernelGGL(k_duplex_events<false>, dim3(blocks_for(c->n, 16)), dim3(256), 0, st, A);
                       },
                       [&](int64_t cap) { reserve_for_keys(c, cap); });
        if (K.over) {                                    // (the front stays as the decode left it: the next run over it clears it)
            *overflow = true;
            return HIMUT_OK;
        }
        hipLaunchKernelGGL(k_duplex_overlap, dim3(blocks_for(c->n, 4)), dim3(256), 0, st, A);
        if (K.n > 0) {
            sort_with_tmp(D.d_sorttmp, true, [&](void* tmp, size_t& bytes) { return sort_keys(c, tmp, bytes, K.n); });
            sort_with_tmp(D.d_rletmp, true, [&](void* tmp, size_t& bytes) { return encode_keys(c, tmp, bytes, K.n); });
            ncand = read_word(c, dsc + DX_W_NCAND);
        }
        reserve_for_candidates(c, ncand);
        if (ncand > 0) {
            hipLaunchKernelGGL(k_duplex_sites, dim3(blocks_for(ncand, 256)), dim3(256), 0, st, D.d_uniq.as<uint64_t>(), ncand,
                               D.sites.d_pos.as<int32_t>(), D.sites.d_code.as<uint8_t>());
            HCHECK(hipMemsetAsync(D.d_tally.p, 0, (size_t)ncand * 8, st));
            A.uniq = D.d_uniq.as<uint64_t>(); A.ncand = ncand; A.tally = D.d_tally.as<uint32_t>();
            hipLaunchKernelGGL(k_duplex_events<true>, dim3(blocks_for(c->n, 16)), dim3(256), 0, st, A);
        }
    } else {
        reserve_for_candidates(c, 0);
    }
    stage_event(c, EV_HAP, 2, st);

    SitesTotals T;
    if (int rc = sites_back(c, D.sites, SF, ncand, overflow, &T)) return rc;
    if (*overflow) return HIMUT_OK;
    // (behind the front's tail, so outside ms_total: a copy of 80 bytes per candidate)
    if (ncand > 0)
        hipLaunchKernelGGL(k_duplex_records, dim3(blocks_for(ncand, 256)), dim3(256), 0, st, D.sites.d_recs.as<himut_site_record>(),
                           D.d_nds.as<uint32_t>(), D.d_tally.as<uint32_t>(), ncand, D.d_recs.as<himut_duplex_record>());
    unsigned long long w[DX_WORDS] = {};
    if (c->n > 0) HCHECK(hipMemcpyAsync(w, dsc, sizeof(w), hipMemcpyDeviceToHost, st));
    HCHECK(hipStreamSynchronize(st));
    if (!spec_keys && c->n > 0) D.cap_keys = K.cap;

    int64_t log[40] = {};
    for (int k = 0; k < 3; k++) log[k] = (int64_t)w[DX_W_READS + k];
    for (int k = 0; k < 20; k++) log[3 + k] = (int64_t)w[DX_W_PAIRS + k];      // pairs .. ds_events_in_chunk
    for (int k = 0; k < 12; k++) { D.ss[k] = (int64_t)w[DX_W_SS + k]; log[23] += D.ss[k]; }
    log[24] = (int64_t)w[DX_W_DSBASES]; log[25] = (int64_t)w[DX_W_OVERLAP];
    log[26] = ncand;
    for (int k = 0; k < 12; k++) log[27 + k] = T.log[2 + k];                    // Germline, then the eleven verdicts
    D.out.n = ncand;
    take_log(D.out, log);
    front_stats(c, DUPLEX_STAGES, sizeof(DUPLEX_STAGES) / sizeof(DUPLEX_STAGES[0]), positions, ncand, ncand, T.nslots);
    return HIMUT_OK;
}

}  // namespace

extern "C" {

int himut_run_duplex(himut_ctx* c, const int32_t* mate, int64_t n_mate, const himut_duplex_params* p) {
    if (!c) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int {
        if (int rc = check_run_inputs(c, NEED_PARAMS | NEED_LUT | NEED_READS | NEED_REGIONS)) return rc;
        if (int rc = check_mate(c, mate, n_mate, p)) return rc;
        himut_ctx::Duplex& D = c->duplex;
        begin_run(c, D.out);                             // (the buffers below may move: what the getter served is gone)
        upload(D.d_mate, mate, (size_t)n_mate, c->stream);
        HCHECK(hipStreamSynchronize(c->stream));         // (mate is the caller's)
        return run_repeating(c, [&](bool kept, bool* overflow) { return duplex_once(c, kept, overflow); },
                             [&] { c->duplex.cap_keys = 0; c->duplex.sites.cap_slots = 0; });
    });
}

int himut_get_duplex(himut_ctx* c, const himut_duplex_record** records, int64_t* n, int64_t ss[12], int64_t log[40]) {
    if (!c || !records || !n) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int {
        if (ss) std::copy(c->duplex.ss, c->duplex.ss + 12, ss);
        return get_run_out(c, c->duplex.out, c->duplex.d_recs, records, n, log);
    });
}

}  // extern "C"
