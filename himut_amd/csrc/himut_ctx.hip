// libhimut_hip.so: the context, the setters, the read batch, the chunk tables and the pinned staging windows.  The
// layout of the host side: himut_ctx.h.
#include <hip/hip_runtime.h>

#include <climits>
#include <mutex>

#include "himut_ctx.h"

using namespace himut;

namespace himut {

namespace {

const char* err_text(int code) {
    switch (code) {
        case HIMUT_ERR_CS: return "cs tag cannot be tokenised or disagrees with SEQ/CIGAR";
        case HIMUT_ERR_BASE: return "KeyError: base outside ATGC (util.py:17)";
        case HIMUT_ERR_BQ0: return "ValueError: math domain error (BQ 0 in a candidate column, gtlib.py:64)";
        case HIMUT_ERR_COVER: return "KeyError: hetSNP position missing from tpos2qbase (haplib.py:51)";
        case HIMUT_ERR_DEPTH: return "pile too deep: the contig's candidate columns need more than 2^32 column-store slots";
    }
    return "device error";
}

// the two pinned staging windows of the process, and the context that holds them
void* g_pinned[2] = {nullptr, nullptr};
size_t g_pinned_bytes = 0;
himut_ctx* g_pinned_owner = nullptr;
std::mutex g_pinned_mx;

}  // namespace

int check_device_err(himut_ctx* c, int bits) {
    if (!bits) return HIMUT_OK;
    for (int code = 1; code < 31; code++)
        if (bits & (1 << code)) return fail(c, code, err_text(code));
    return fail(c, HIMUT_ERR_ARG, "device error");
}

int check_run_inputs(himut_ctx* c, unsigned needs) {
    if ((needs & NEED_PARAMS) && !c->have_params) return fail(c, HIMUT_ERR_ARG, "himut_set_params has not been called");
    if ((needs & NEED_LUT) && !c->have_lut) return fail(c, HIMUT_ERR_ARG, "himut_set_gt_lut has not been called");
    if ((needs & NEED_READS) && !c->have_reads) return fail(c, HIMUT_ERR_ARG, "himut_push_reads has not been called");
    if ((needs & NEED_REGIONS) && c->cstart.empty()) return fail(c, HIMUT_ERR_ARG, "himut_set_chunks has not been called: no regions");
    if ((needs & NEED_REFERENCE) && c->reflen <= 0) return fail(c, HIMUT_ERR_ARG, "himut_set_reference has not been called");
    if (needs & NEED_SPANS)
        for (size_t k = 0; k < c->cstart.size(); k++)
            if (c->cstart[k] > c->cend[k]) return fail(c, HIMUT_ERR_CHUNK, "ValueError: invalid coordinates: region start > end");
    return HIMUT_OK;
}

int encode_sites(himut_ctx* c, const char* who, const int32_t* pos1, const uint8_t* ref, const uint8_t* alt, int64_t n_sites,
                 std::vector<uint8_t>* code) {
    auto allele_of = [](uint8_t b) { return b == 'A' ? 0 : b == 'T' ? 1 : b == 'G' ? 2 : b == 'C' ? 3 : -1; };
    code->resize((size_t)n_sites);
    for (int64_t k = 0; k < n_sites; k++) {
        const int ra = allele_of(ref[k]), aa = allele_of(alt[k]);
        if (pos1[k] < 1 || (k && pos1[k] < pos1[k - 1]))
            return fail(c, HIMUT_ERR_ARG, std::string(who) + ": site positions must be 1-based and non-decreasing");
        if (ra < 0 || aa < 0 || ra == aa)
            return fail(c, HIMUT_ERR_ARG, std::string(who) + ": ref and alt must be different upper-case letters of ATGC");
        (*code)[(size_t)k] = (uint8_t)((ra << 2) | aa);
    }
    return HIMUT_OK;
}

int check_scan_inputs(himut_ctx* c, bool need_reference) {
    if (int rc = check_run_inputs(c, NEED_PARAMS | NEED_LUT | NEED_READS | (need_reference ? NEED_REFERENCE : 0u))) return rc;
    const bool phase = c->params.p.phase != 0;
    if (phase && !c->have_phase) return fail(c, HIMUT_ERR_ARG, "phase requested but himut_set_phase has not been called");
    if (phase && (int64_t)c->h_phoff.size() != (int64_t)c->cstart.size() + 1)
        return fail(c, HIMUT_ERR_ARG, "himut_set_phase chunk count differs from himut_set_chunks");
    for (size_t k = 0; k < c->cstart.size(); k++)
        if (c->cstart[k] > c->cend[k]) return fail(c, HIMUT_ERR_CHUNK, "ValueError: invalid coordinates: chunk start > end");
    return HIMUT_OK;
}

bool claim_pinned(himut_ctx* c, bool own_ok) {
    std::lock_guard<std::mutex> lock(g_pinned_mx);
    if (g_pinned_owner && (g_pinned_owner != c || !own_ok)) return false;
    g_pinned_owner = c;
    return true;
}

bool size_pinned(himut_ctx* c, size_t bytes, unsigned flags, void* host[2]) {
    bool grew;
    {
        std::lock_guard<std::mutex> lock(g_pinned_mx);
        grew = g_pinned_bytes < bytes + 4096;
        if (grew) {
            for (int k = 0; k < 2; k++) {
                if (g_pinned[k]) { HCHECK(hipHostFree(g_pinned[k])); g_pinned[k] = nullptr; }
                HCHECK(hipHostMalloc(&g_pinned[k], bytes + 4096, flags));
            }
            g_pinned_bytes = bytes + 4096;
        }
    }
    for (int k = 0; k < 2; k++) {
        host[k] = g_pinned[k];
        if (!c->stage_copied[k]) HCHECK(hipEventCreateWithFlags(&c->stage_copied[k], hipEventDisableTiming));
        if (!c->stage_parsed[k]) HCHECK(hipEventCreateWithFlags(&c->stage_parsed[k], hipEventDisableTiming));
        c->d_stage[k].reserve(bytes + 4096);
    }
    return grew;
}

void release_pinned(himut_ctx* c) {
    std::lock_guard<std::mutex> lock(g_pinned_mx);
    if (g_pinned_owner == c) g_pinned_owner = nullptr;
}

void sorted_regions(const std::vector<int32_t>& cs, const std::vector<int32_t>& ce, std::vector<int32_t>* sstart,
                    std::vector<int32_t>* spmax, std::vector<int32_t>* sidx) {
    const size_t n = cs.size();
    std::vector<int32_t> order(n);
    for (size_t k = 0; k < n; k++) order[k] = (int32_t)k;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return cs[(size_t)a] < cs[(size_t)b]; });
    sstart->resize(n);
    spmax->resize(n);
    int32_t run = INT32_MIN;
    for (size_t k = 0; k < n; k++) {
        (*sstart)[k] = cs[(size_t)order[k]];
        run = std::max(run, ce[(size_t)order[k]]);
        (*spmax)[k] = run;
    }
    if (sidx) sidx->swap(order);
}

ChunkTables upload_chunks(himut_ctx* c, const std::vector<int32_t>& cs, const std::vector<int32_t>& ce) {
    ChunkTables T;
    const int TP = PD_TP;  // tiles are only used by the dense pile kernel
    const int64_t n = (int64_t)cs.size();
    T.n = n;
    if (c->tables_valid && cs == c->up_cs && ce == c->up_ce) {   // same chunks, same reads: the tables are on the device
        T.positions = c->up_positions; T.n_tiles = c->up_tiles; T.npairs = c->up_pairs; T.maxpairs = c->up_maxpairs;
        return T;
    }
    c->maskoff.assign(n + 1, 0);
    c->tileoff.assign(n + 1, 0);
    for (int64_t k = 0; k < n; k++) {
        int64_t span = (int64_t)ce[k] - cs[k] + 1;
        c->maskoff[k + 1] = c->maskoff[k] + span;
        c->tileoff[k + 1] = c->tileoff[k] + (span + TP - 1) / TP;
    }
    T.positions = c->maskoff[n];
    T.n_tiles = c->tileoff[n];
    std::vector<int32_t> sstart, sidx, spmax;
    sorted_regions(cs, ce, &sstart, &spmax, &sidx);
    // read windows per chunk: [first read whose running max tend > start, first read with tstart >= end)
    std::vector<int64_t> rlo(n), rhi(n), pairoff(n + 1, 0);
    for (int64_t k = 0; k < n; k++) {
        rlo[k] = std::upper_bound(c->h_prefmax.begin(), c->h_prefmax.end(), cs[k]) - c->h_prefmax.begin();
        rhi[k] = std::lower_bound(c->h_tstart.begin(), c->h_tstart.end(), ce[k]) - c->h_tstart.begin();
        if (rhi[k] < rlo[k]) rhi[k] = rlo[k];
        pairoff[k + 1] = pairoff[k] + (rhi[k] - rlo[k]);
        T.maxpairs = std::max<int64_t>(T.maxpairs, rhi[k] - rlo[k]);
    }
    T.npairs = pairoff[n];
    // look-up hint: for each 16-kb block of positions, the number of sorted starts <= block start
    int32_t maxend = 0;
    for (int64_t k = 0; k < n; k++) maxend = std::max(maxend, ce[k]);
    c->nhint = ((int64_t)maxend >> CHUNK_HINT_SHIFT) + 2;
    std::vector<int32_t> hint((size_t)c->nhint);
    {
        int64_t j = 0;
        for (int64_t b = 0; b < c->nhint; b++) {
            const int64_t p = b << CHUNK_HINT_SHIFT;
            while (j < n && (int64_t)sstart[j] <= p) j++;
            hint[(size_t)b] = (int32_t)j;
        }
    }
    std::vector<ChunkRec> crec((size_t)n);
    for (int64_t k = 0; k < n; k++) {
        const int32_t ci = sidx[k];
        crec[k].start = cs[ci]; crec[k].end = ce[ci]; crec[k].idx = ci; crec[k].pmaxend = spmax[k];
        crec[k].maskoff = c->maskoff[ci]; crec[k].pairbase = pairoff[ci] - rlo[ci];
    }
    // candidates come out of the mask in (chunk, tpos) order; that is the record order when
    // no chunk starts before its predecessor's end (the reference's chunking shares only the edge)
    c->chunks_in_order = true;
    for (int64_t k = 1; k < n; k++) if (cs[k] < ce[k - 1]) c->chunks_in_order = false;
    // mask tiles (MASK_TILE_CELLS cells each): the chunk their first cell belongs to
    const int64_t ntile = std::max<int64_t>(1, ((int64_t)T.positions + MASK_TILE_CELLS - 1) / MASK_TILE_CELLS);
    std::vector<MaskTile> mtile((size_t)ntile);
    {
        int64_t ck = 0;
        for (int64_t b = 0; b < ntile; b++) {
            const int64_t cell = b * MASK_TILE_CELLS;
            while (ck + 1 < n && c->maskoff[ck + 1] <= cell) ck++;
            MaskTile& m = mtile[(size_t)b];
            m.ck0 = (int32_t)ck; m.start0 = n > 0 ? cs[ck] : 0;
            m.off0 = n > 0 ? c->maskoff[ck] : 0; m.off1 = n > 0 ? c->maskoff[ck + 1] : 0; m.pad = 0;
        }
    }
    // chunks in order: the mask is indexed by column rank, and k_mask_emit wants, per 256-position block, the first
    // chunk that ends at or behind the block's first tpos (the ends are in order too); behind the last end: n
    std::vector<int32_t> blkchunk;
    if (c->chunks_in_order) {
        blkchunk.resize((size_t)(((int64_t)maxend >> WIN_SHIFT) + 2));
        int64_t k = 0;
        for (size_t b = 0; b < blkchunk.size(); b++) {
            const int64_t t0 = ((int64_t)b << WIN_SHIFT) + 1;
            while (k < n && (int64_t)ce[k] < t0) k++;
            blkchunk[b] = (int32_t)k;
        }
    }
    c->n_blkchunk = (int64_t)blkchunk.size();
    hipStream_t st = c->stream;
    upload(c->d_blkchunk, blkchunk, st);
    upload(c->d_hint, hint, st);
    upload(c->d_crec, crec, st);
    upload(c->d_mtile, mtile, st);
    upload(c->d_cstart, cs, st); upload(c->d_cend, ce, st);
    upload(c->d_maskoff, c->maskoff, st); upload(c->d_tileoff, c->tileoff, st);
    upload(c->d_sstart, sstart, st); upload(c->d_sidx, sidx, st); upload(c->d_spmax, spmax, st);
    upload(c->d_rlo, rlo, st); upload(c->d_rhi, rhi, st); upload(c->d_pairoff, pairoff, st);
    HCHECK(hipStreamSynchronize(st));  // the host vectors above go out of scope
    c->up_cs = cs; c->up_ce = ce; c->tables_valid = true;
    c->up_positions = T.positions; c->up_tiles = T.n_tiles; c->up_pairs = T.npairs; c->up_maxpairs = T.maxpairs;
    return T;
}

}  // namespace himut

extern "C" {

int himut_abi_version(void) { return HIMUT_ABI_VERSION; }

__global__ void k_warm(int* p) { if (p) *p = 0; }

int himut_create(int device, himut_ctx** out) {
    if (!out) return HIMUT_ERR_ARG;
    *out = nullptr;
    himut_ctx* c = new (std::nothrow) himut_ctx();
    if (!c) return HIMUT_ERR_NOMEM;
    c->device = device;
    int rc = guarded(c, [&]() -> int {
        int ndev = 0;
        HCHECK(hipGetDeviceCount(&ndev));
        if (device < 0 || device >= ndev) return fail(c, HIMUT_ERR_ARG, "no such HIP device");
        HCHECK(hipSetDevice(device));
        hipDeviceProp_t prop;
        HCHECK(hipGetDeviceProperties(&prop, device));
        c->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        HCHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        HCHECK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
        for (auto& e : c->ev) HCHECK(hipEventCreate(&e));
        HCHECK(hipHostMalloc(&c->h_scalars, sizeof(Scalars), hipHostMallocDefault));
        // the library's code object is loaded with the first launch (tens of milliseconds): here, not in the first
        // contig's ingest or scan
        hipLaunchKernelGGL(k_warm, dim3(1), dim3(64), 0, c->stream, (int*)nullptr);
        HCHECK(hipStreamSynchronize(c->stream));
        return HIMUT_OK;
    });
    if (rc) {
        static thread_local std::string last;
        last = c->err;
        delete c;
        return rc;
    }
    *out = c;
    return HIMUT_OK;
}

void himut_destroy(himut_ctx* c) {
    if (!c) return;
    release_pinned(c);
    (void)hipSetDevice(c->device);
    if (c->stream) { (void)hipStreamSynchronize(c->stream); }
    if (c->side) { (void)hipStreamSynchronize(c->side); (void)hipStreamDestroy(c->side); }
    for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->h_scalars) (void)hipHostFree(c->h_scalars);
    for (int k = 0; k < 2; k++) {
        if (c->stage_copied[k]) (void)hipEventDestroy(c->stage_copied[k]);
        if (c->stage_parsed[k]) (void)hipEventDestroy(c->stage_parsed[k]);
    }
    delete c;
}

int himut_set_stage_timing(himut_ctx* c, int level) {
    if (!c) return HIMUT_ERR_ARG;
    if (level < 0 || level > 2) return fail(c, HIMUT_ERR_ARG, "stage timing level must be 0, 1 or 2");
    c->timing = level;
    return HIMUT_OK;
}

const char* himut_last_error(const himut_ctx* c) { return c ? c->err.c_str() : "null context"; }

int himut_set_params(himut_ctx* c, const himut_params* p) {
    if (!c || !p) return HIMUT_ERR_ARG;
    c->params.p = *p;
    c->have_params = true;
    return HIMUT_OK;
}

int himut_set_gt_lut(himut_ctx* c, const double* hom, const double* het, const double* err_, int n_bq, const double prior[4]) {
    if (!c || !hom || !het || !err_ || !prior || n_bq < 1 || n_bq > 256) return fail(c, HIMUT_ERR_ARG, "bad LUT arguments");
    return guarded(c, [&]() -> int {
        HCHECK(hipSetDevice(c->device));
        GtLut L;
        for (int k = 0; k < 256; k++) {
            const int s = k < n_bq ? k : n_bq - 1;
            L.t[0][k] = hom[s]; L.t[1][k] = het[s]; L.t[2][k] = err_[s];
        }
        for (int k = 0; k < 4; k++) L.prior[k] = prior[k];
        c->d_lut.reserve(sizeof(GtLut));
        HCHECK(hipMemcpyAsync(c->d_lut.p, &L, sizeof(GtLut), hipMemcpyHostToDevice, c->stream));
        HCHECK(hipStreamSynchronize(c->stream));
        c->have_lut = true;
        return HIMUT_OK;
    });
}

int himut_set_chunks(himut_ctx* c, const int32_t* start, const int32_t* end, int64_t n) {
    if (!c || n < 0 || (n > 0 && (!start || !end))) return fail(c, HIMUT_ERR_ARG, "bad chunk arguments");
    if (n >= (1 << 24)) return fail(c, HIMUT_ERR_ARG, "too many chunks");
    c->cstart.assign(start, start + n);
    c->cend.assign(end, end + n);
    return HIMUT_OK;
}

int himut_set_site_set(himut_ctx* c, int which, const uint64_t* keys, int64_t n) {
    if (!c || (which != 0 && which != 1) || n < 0 || (n > 0 && !keys)) return fail(c, HIMUT_ERR_ARG, "bad site-set arguments");
    for (int64_t k = 1; k < n; k++)
        if (keys[k - 1] > keys[k]) return fail(c, HIMUT_ERR_ARG, "site-set keys must be sorted ascending");
    return guarded(c, [&]() -> int {
        HCHECK(hipSetDevice(c->device));
        DevBuf& b = which == 0 ? c->d_pon : c->d_com;
        upload(b, keys, (size_t)n, c->stream);
        (which == 0 ? c->h_pon : c->h_com).assign(keys, keys + n);
        (which == 0 ? c->npon : c->ncom) = n;
        // position bitmap over both sets: lets a candidate skip the two binary searches
        uint64_t maxpos = 0;
        for (const auto* v : {&c->h_pon, &c->h_com})
            if (!v->empty()) maxpos = std::max<uint64_t>(maxpos, v->back() >> 4);
        std::vector<uint32_t> bits((size_t)(maxpos >> 5) + 2, 0u);
        for (const auto* v : {&c->h_pon, &c->h_com})
            for (uint64_t k : *v) bits[(size_t)((k >> 4) >> 5)] |= 1u << ((k >> 4) & 31);
        c->nposbits = (c->h_pon.empty() && c->h_com.empty()) ? 0 : (int64_t)maxpos + 1;
        upload(c->d_posbits, bits, c->stream);
        HCHECK(hipStreamSynchronize(c->stream));
        return HIMUT_OK;
    });
}

int himut_set_phase(himut_ctx* c, const int64_t* off, const int32_t* hpos, const uint8_t* href, const uint8_t* halt,
                    const uint8_t* hbit, int64_t n_chunks) {
    if (!c || !off || n_chunks < 0) return fail(c, HIMUT_ERR_ARG, "bad phase arguments");
    return guarded(c, [&]() -> int {
        HCHECK(hipSetDevice(c->device));
        const int64_t m = off[n_chunks];
        c->h_phoff.assign(off, off + n_chunks + 1);
        upload(c->d_phoff, off, (size_t)n_chunks + 1, c->stream);
        upload(c->d_hpos, hpos, (size_t)m, c->stream);
        upload(c->d_href, href, (size_t)m, c->stream);
        upload(c->d_halt, halt, (size_t)m, c->stream);
        upload(c->d_hbit, hbit, (size_t)m, c->stream);
        HCHECK(hipStreamSynchronize(c->stream));
        c->have_phase = true;
        return HIMUT_OK;
    });
}

int himut_push_reads(himut_ctx* c, const himut_read_batch* b) {
    if (!c || !b || b->n_reads < 0) return fail(c, HIMUT_ERR_ARG, "bad read batch");
    const int64_t n = b->n_reads;
    if (n > 0 && (!b->tstart || !b->tend || !b->qstart || !b->qlen || !b->mapq || !b->flag || !b->qid || !b->qoff ||
                  !b->cs_off || !b->seq || !b->bq || !b->cs))
        return fail(c, HIMUT_ERR_ARG, "read batch has null arrays");
    // host-side shape checks: everything the kernels index with must be in range
    int64_t bases = 0;
    bool unique = true;
    for (int64_t i = 0; i < n; i++) {
        if (i > 0 && b->tstart[i] < b->tstart[i - 1]) return fail(c, HIMUT_ERR_ARG, "reads are not coordinate sorted");
        if (b->qoff[i] < 0 || (b->qoff[i] & 31) || b->qlen[i] < 0 || b->qoff[i] + (((int64_t)b->qlen[i] + 31) & ~(int64_t)31) > b->bq_bytes ||
            (b->qoff[i] + (((int64_t)b->qlen[i] + 31) & ~(int64_t)31)) / 2 > b->seq_bytes)
            return fail(c, HIMUT_ERR_ARG, "read offsets exceed the sequence / quality buffers");
        if (b->cs_off[i] < 0 || b->cs_off[i + 1] < b->cs_off[i] || b->cs_off[i + 1] > b->cs_bytes)
            return fail(c, HIMUT_ERR_ARG, "cs offsets exceed the cs buffer");
        if (b->tend[i] < b->tstart[i] || b->qstart[i] < 0 || b->qstart[i] > b->qlen[i])
            return fail(c, HIMUT_ERR_ARG, "read coordinates are inconsistent");
        if (b->qid[i] < 0 || b->qid[i] >= n) return fail(c, HIMUT_ERR_ARG, "qid out of range");
        if (b->qid[i] != i) unique = false;
        bases += b->qlen[i];
    }
    return guarded(c, [&]() -> int {
        HCHECK(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        c->n = n; c->cs_bytes = b->cs_bytes; c->seq_bytes = b->seq_bytes; c->bq_bytes = b->bq_bytes; c->read_bases = bases;
        c->unique_qnames = unique;
        c->h_tstart.assign(b->tstart, b->tstart + n);
        c->h_tend.assign(b->tend, b->tend + n);
        c->h_prefmax.resize((size_t)n);
        int32_t run = INT32_MIN;
        for (int64_t i = 0; i < n; i++) { run = std::max(run, b->tend[i]); c->h_prefmax[(size_t)i] = run; }
        upload(c->d_tstart, b->tstart, (size_t)n, st); upload(c->d_tend, b->tend, (size_t)n, st);
        upload(c->d_qstart, b->qstart, (size_t)n, st); upload(c->d_qlen, b->qlen, (size_t)n, st);
        upload(c->d_mapq, b->mapq, (size_t)n, st); upload(c->d_flag, b->flag, (size_t)n, st);
        upload(c->d_qid, b->qid, (size_t)n, st); upload(c->d_qoff, b->qoff, (size_t)n, st);
        upload(c->d_csoff, b->cs_off, (size_t)n + 1, st);
        upload(c->d_seq, b->seq, (size_t)b->seq_bytes, st); upload(c->d_bq, b->bq, (size_t)b->bq_bytes, st);
        // k_parse_cs takes the text 1 KB at a time, 16 bytes per lane, whatever is left of the tag: the last read's
        // window runs up to 1 KB past the end of the text
        c->d_cs.reserve((size_t)b->cs_bytes + 2048);
        upload(c->d_cs, b->cs, (size_t)b->cs_bytes, st);
        upload(c->d_prefmax, c->h_prefmax, st);
        // long-form cs ('=' operations) needs one extra checking kernel; find out once, on the host
        c->any_longcs = memchr(b->cs, '=', (size_t)b->cs_bytes) != nullptr;
        HCHECK(hipStreamSynchronize(st));
        c->have_reads = true;
        forget_reads(c);
        return HIMUT_OK;
    });
}

// tstart, tend, the SAM flag and mapq of the context's reads, pushed or ingested, back on the host
int himut_get_read_info(himut_ctx* c, int32_t* tstart, int32_t* tend, uint16_t* flag, uint8_t* mapq) {
    if (!c) return HIMUT_ERR_ARG;
    return guarded(c, [&]() -> int {
        if (int rc = check_run_inputs(c, NEED_READS)) return rc;
        HCHECK(hipSetDevice(c->device));
        const size_t n = (size_t)c->n;
        if (!n) return HIMUT_OK;
        HCHECK(hipStreamSynchronize(c->stream));
        if (tstart) HCHECK(hipMemcpy(tstart, c->d_tstart.p, n * 4, hipMemcpyDeviceToHost));
        if (tend) HCHECK(hipMemcpy(tend, c->d_tend.p, n * 4, hipMemcpyDeviceToHost));
        if (flag) HCHECK(hipMemcpy(flag, c->d_flag.p, n * 2, hipMemcpyDeviceToHost));
        if (mapq) HCHECK(hipMemcpy(mapq, c->d_mapq.p, n, hipMemcpyDeviceToHost));
        return HIMUT_OK;
    });
}

}  // extern "C"
