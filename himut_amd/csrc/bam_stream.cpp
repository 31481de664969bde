// Streaming ingest of ONE contig for the device-side record parser (libhimut_hip.so: himut_ingest_*): the host's part
// is what has to be sequential or is cheap -- block inflate (thread pool) straight into a caller's (pinned) buffer,
// the hop from length field to length field, the read-name table -- and the device does the rest (CIGAR walk, tag
// scan, placement, byte copies).  With an index beside the file (x.bam.bai) only the contig's own BGZF blocks are
// inflated; without one the blocks in front of it are inflated and hopped over.
#include <memory>
#include <unordered_map>

#include "host_bam.h"

namespace {

struct BamStream {
    Bgzf z;
    BamHeader hdr;
    size_t first_block = 0, first_skip = 0;            // where the first record of the file starts
    bool have_bai = false;
    std::vector<std::pair<uint64_t, uint64_t>> ref_range;   // per contig: virtual offsets of its first record / end of its last
    int32_t target = -1;
    size_t blk = 0, blk_end = 0, skip = 0;
    std::vector<uint8_t> carry;
    std::unordered_map<std::string, int32_t> names;
    int64_t nkept = 0;
    bool keep_names = false, names_kept = false;   // bam_stream_keep_names: asked for; the selected contig's are being kept
    std::vector<std::string> kept_names;          // the kept records' names by ordinal (bam_stream_read_name)
    bool done = false, unique = true;
    bool cigar_sums = false;              // bam_stream_sum_cigar: sums[1] of stream_next counts CIGAR bytes, not auxiliary bytes
    std::string err;
    double t_inflate = 0, t_hop = 0;      // HIMUT_INGEST_PROFILE
    int64_t n_windows = 0, inflated_bytes = 0;   // inflated_bytes: what this stream has inflated since it was opened (header blocks excluded)
    std::future<std::string> inflating;   // the window being inflated in the background (stream_prefetch)
    std::vector<size_t> inf_off;
    size_t inf_tot = 0;
    std::unique_ptr<uint32_t[]> pump_off[2];   // bam_stream_pump's record lists: handed to the device asynchronously, so
    std::unique_ptr<int32_t[]> pump_qid[2];    // they live as long as the stream, not as long as the call.  Sized for the
    int64_t pump_cap = 0;                      // shortest legal records and not cleared: only what a window lists is touched
    bool ready = false;                   // a window is inflated and waits for its hop (stream_wait)
    size_t ready_tot = 0;
};
constexpr size_t BAM_STREAM_HEAD = (size_t)4 << 20;

// The index beside the file (.bai, SAM specification section 5.2), slurped and walked once.  ``hints``: file offsets at
// which it says BGZF blocks start (chunk begins and linear-index entries), sorted; only hints for the parallel block
// scan and best effort: an index that breaks off gives those read so far, a wrong or stale one costs nothing but the
// serial scan.  ``ranges``: per contig the virtual offsets of its first record and of the end of its last (~0, 0: no
// records); all or nothing: ``complete`` only when the whole index was walked, and the caller compares their number
// with the header's n_ref.
struct BaiIndex {
    std::vector<size_t> hints;
    std::vector<std::pair<uint64_t, uint64_t>> ranges;
    bool complete = false;
};

BaiIndex read_bai(const std::string& path) {
    BaiIndex X;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return X;
    std::vector<uint8_t> d;
    uint8_t tmp[1 << 16];
    size_t k;
    while ((k = fread(tmp, 1, sizeof(tmp), f)) > 0) d.insert(d.end(), tmp, tmp + k);
    fclose(f);
    size_t p = 0;
    auto need = [&](uint64_t n) { return p + n <= d.size(); };
    auto r32 = [&]() { const uint32_t v = le32(&d[p]); p += 4; return v; };
    auto r64 = [&]() { uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)d[p + i] << (8 * i); p += 8; return v; };
    auto walk = [&]() {                                         // false where the index breaks off
        if (!need(8) || memcmp(d.data(), "BAI\1", 4) != 0) return false;
        p = 4;
        const uint32_t n = r32();
        for (uint32_t i = 0; i < n; i++) {
            std::pair<uint64_t, uint64_t> range(~0ull, 0ull);
            if (!need(4)) return false;
            const uint32_t nbin = r32();
            for (uint32_t b = 0; b < nbin; b++) {
                if (!need(8)) return false;
                const uint32_t bin = r32(), nch = r32();
                if (!need(16ull * nch)) return false;
                for (uint32_t c = 0; c < nch; c++) {
                    const uint64_t beg = r64(), end = r64();
                    if (bin == 37450) continue;                 // samtools' metadata pseudo-bin
                    X.hints.push_back((size_t)(beg >> 16));
                    range.first = std::min(range.first, beg);
                    range.second = std::max(range.second, end);
                }
            }
            if (!need(4)) return false;
            const uint32_t nint = r32();
            if (!need(8ull * nint)) return false;
            for (uint32_t c = 0; c < nint; c++) { const uint64_t v = r64(); if (v) X.hints.push_back((size_t)(v >> 16)); }
            X.ranges.push_back(range);
        }
        return true;
    };
    X.complete = walk();
    std::sort(X.hints.begin(), X.hints.end());
    X.hints.erase(std::unique(X.hints.begin(), X.hints.end()), X.hints.end());
    return X;
}

// A window buffer = BAM_STREAM_HEAD bytes of head room + the inflated blocks.  The inflate of window k + 1 (thread pool,
// started by stream_prefetch, running in the background) overlaps the hop over window k and its hand-over to the
// GPU; the partial record that window k ends with is then put in FRONT of window k + 1's bytes, in the head room, so
// the inflate never has to wait for it.

// Starts inflating the next blocks of the contig into buf + HEAD (as many as fit cap - HEAD).  Returns 1 when an
// inflate is in flight, 0 when the contig has no more blocks, -2 on error.  One prefetch may be in flight.
int stream_prefetch(BamStream* S, uint8_t* buf, int64_t cap) {
    if (S->inflating.valid()) { S->err = "a prefetch is in flight already"; return -2; }
    if (S->done || S->blk >= S->blk_end) return 0;
    const auto& B = S->z.blocks;
    S->inf_off.clear();
    size_t tot = 0, b0 = S->blk, b1 = S->blk;
    while (b1 < S->blk_end && (int64_t)(BAM_STREAM_HEAD + tot + B[b1].isize) <= cap) { S->inf_off.push_back(tot); tot += B[b1].isize; b1++; }
    if (b1 == b0) { S->err = "ingest window smaller than a BGZF block"; return -2; }
    S->blk = b1;
    S->inf_tot = tot; S->inflated_bytes += (int64_t)tot;
    uint8_t* dst = buf + BAM_STREAM_HEAD;
    S->inflating = std::async(std::launch::async, [S, b0, b1, dst]() {
        const double t0 = now_s();
        std::string e = S->z.inflate_blocks(b0, b1, dst, 0, &S->inf_off);
        S->t_inflate += now_s() - t0; S->n_windows++;
        return e;
    });
    return 1;
}

// Waits for the inflate in flight.  Returns 1 when a window is now ready for stream_next, 0 when none was in flight,
// -2 on error.  After it the next prefetch may be started BEFORE the hop over this window (stream_next), so the
// pool never idles while one thread walks the records.
int stream_wait(BamStream* S) {
    if (S->ready) return 1;
    if (!S->inflating.valid()) return 0;
    const std::string e = S->inflating.get();
    if (!e.empty()) { S->err = e; return -2; }
    S->ready = true; S->ready_tot = S->inf_tot;
    return 1;
}

// Finishes the window whose inflate stream_prefetch(buf) started (or, with none in flight, inflates one now): hops
// over the records and lists the kept ones (this contig, mapped): rec_off[k] = offset of record k's body (behind its
// length field) from buf + *start, qid[k] = index of the first kept record with the same read name.  The records occupy
// *nbytes bytes from buf + *start.  sums: of the kept records, query lengths rounded up to 32 and bytes of the auxiliary
// fields (after bam_stream_sum_cigar(h, 1): bytes of the CIGARs, what an ingest that derives the cs text keeps).
// Returns the number of kept records (0: a window of other contigs' records, go on), -1 at the end of the contig, -2
// on error.  Like the two above it is called by pump_run alone; bam_stream_pump words what any of them throws.
int64_t stream_next(BamStream* S, uint8_t* buf, int64_t cap, uint32_t* rec_off, int32_t* qid, int64_t rec_cap, int64_t* start,
                    int64_t* nbytes, int64_t* sums) {
    *nbytes = 0; *start = 0;
    sums[0] = sums[1] = 0;
    if (!S->ready && !S->inflating.valid()) {
        if (S->done) return -1;
        const int r = stream_prefetch(S, buf, cap);
        if (r < 0) return -2;
        if (r == 0 && S->carry.empty()) return -1;
    }
    if (!S->ready && stream_wait(S) < 0) return -2;
    const size_t tot = S->ready ? S->ready_tot : 0;        // no window: only what the last one left is hopped over
    S->ready = false;
    const double t_h0 = now_s();
    const size_t c = S->carry.size();
    if (c > BAM_STREAM_HEAD) { S->err = "a BAM record is larger than the head room of the ingest window"; return -2; }
    uint8_t* dst = buf + BAM_STREAM_HEAD - c;
    if (c) memcpy(dst, S->carry.data(), c);
    S->carry.clear();
    const size_t nb = c + tot;
    size_t pos = S->skip;
    S->skip = 0;
    const size_t first = pos;
    int64_t n = 0;
    const char* bad = nullptr;                             // a kept record whose parts outgrow its length field
    const char* too_short = hop_records(dst, pos, nb, [&](const uint8_t* rec, uint32_t bs) {
        if (n >= rec_cap) return false;
        const int32_t ref_id = (int32_t)le32(rec);
        const uint16_t flag = le16(rec + 14);
        if (ref_id > S->target || ref_id < 0) { S->done = true; return false; }   // coordinate sorted: the contig is over
        if (ref_id == S->target && !(flag & 4)) {
            const uint64_t fixed = record_fixed_bytes(rec);
            if (fixed > bs) { bad = "malformed BAM record"; return false; }
            const size_t l_qname = rec[8];
            const char* qn = (const char*)rec + 32;
            auto it = S->names.emplace(std::string(qn, strnlen(qn, l_qname)), (int32_t)S->nkept);
            if (!it.second) S->unique = false;
            if (S->names_kept) S->kept_names.push_back(it.first->first);
            const uint64_t n_cigar = le16(rec + 12), l_seq = le32(rec + 16);
            sums[0] += (int64_t)((l_seq + 31) & ~(uint64_t)31);
            sums[1] += S->cigar_sums ? (int64_t)(4 * n_cigar) : (int64_t)(bs - fixed);
            rec_off[n] = (uint32_t)(pos + 4 - first);
            qid[n] = it.first->second;
            S->nkept++; n++;
        }
        return true;
    });
    if (too_short || bad) { S->err = too_short ? too_short : bad; return -2; }
    *start = (int64_t)(BAM_STREAM_HEAD - c + first);
    *nbytes = (int64_t)(pos - first);
    S->t_hop += now_s() - t_h0;
    // nothing more comes once every block is taken AND no window is being inflated or waits for its hop (the next
    // prefetch may have been started before this hop)
    const bool last = S->blk >= S->blk_end && !S->inflating.valid() && !S->ready;
    if (!S->done) {
        if (pos < nb) S->carry.assign(dst + pos, dst + nb);
        if (last && !S->carry.empty() && n < rec_cap) {
            // the last block ended inside a record: an indexed range ends with the contig's last record, so what is
            // left belongs to the next contig; without an index the file is truncated
            if (!S->have_bai && S->carry.size() >= 4) { S->err = "truncated BAM record"; return -2; }
            S->carry.clear();
        }
    }
    if (n > 0) return n;
    if (S->done || (last && S->carry.empty())) return -1;
    return 0;
}

typedef int (*ingest_wait_fn)(void*, int);
typedef int (*ingest_window_fn)(void*, int, int64_t, int64_t, const uint32_t*, const int32_t*, int64_t, int64_t, int64_t);

int pump_run(BamStream* S, void* ctx, ingest_wait_fn wait, ingest_window_fn window, uint8_t* buf0, uint8_t* buf1, int64_t cap, int64_t rec_cap) {
    uint8_t* bufs[2] = {buf0, buf1};
    if (rec_cap > S->pump_cap) {
        for (int k = 0; k < 2; k++) { S->pump_off[k].reset(new uint32_t[(size_t)rec_cap]); S->pump_qid[k].reset(new int32_t[(size_t)rec_cap]); }
        S->pump_cap = rec_cap;
    }
    uint32_t* rec_off[2] = {S->pump_off[0].get(), S->pump_off[1].get()};
    int32_t* qid[2] = {S->pump_qid[0].get(), S->pump_qid[1].get()};
    int slot = 0;
    const bool prof = S->z.env.profile;
    double t_wait_inf = 0, t_wait_dev = 0, t_window = 0, t_first_window = 0, t_hop0 = S->t_hop;
    int64_t nwin = 0;
    if (stream_prefetch(S, bufs[0], cap) < 0) return -2;
    for (;;) {
        // window `slot` is inflated: the pool goes on with the next one (into the other buffer, once its bytes of two
        // windows ago have left the host) while this thread hops over the records and hands the window to the GPU
        double t0 = prof ? now_s() : 0;
        if (stream_wait(S) < 0) return -2;
        double t1 = prof ? now_s() : 0;
        int rc = wait(ctx, slot ^ 1);
        if (rc) return rc;
        if (prof) { t_wait_inf += t1 - t0; t_wait_dev += now_s() - t1; }
        if (stream_prefetch(S, bufs[slot ^ 1], cap) < 0) return -2;
        int64_t start = 0, nbytes = 0, sums[2] = {0, 0};
        const int64_t n = stream_next(S, bufs[slot], cap, rec_off[slot], qid[slot], rec_cap, &start, &nbytes, sums);
        if (n == -1) break;
        if (n < 0) return -2;
        t0 = prof ? now_s() : 0;
        if (n > 0 && (rc = window(ctx, slot, start, nbytes, rec_off[slot], qid[slot], n, sums[0], sums[1])) != 0) return rc;
        if (prof) { const double dt = now_s() - t0; t_window += dt; if (!nwin) t_first_window = dt; nwin++; }
        slot ^= 1;
    }
    if (prof)
        fprintf(stderr, "pump (s): waiting for inflate %.3f, for the device %.3f, hop %.3f, handing over %.3f (first window %.3f) in %lld windows\n",
                t_wait_inf, t_wait_dev, S->t_hop - t_hop0, t_window, t_first_window, (long long)nwin);
    return 0;
}

}  // namespace

extern "C" {

// Opens the file with `threads` inflate threads (0: HIMUT_INGEST_THREADS, else one per hardware thread, at most 32) and
// reads its header.  Returns a handle (never null); check bam_stream_error().
void* bam_stream_open(const char* path, int threads) {
    BamStream* S = new BamStream();
    try {
        const IngestEnv env;
        if (threads <= 0) threads = env.default_threads(32);
        Bgzf& z = S->z;
        BaiIndex index;
        if (!env.no_index) index = read_bai(std::string(path) + ".bai");
        if (!z.open(path, threads, env, &index.hints)) { S->err = z.err; return S; }
        // the header sits in the first block or two: they are inflated one at a time, not a window at a time
        size_t consumed = 0, hb_next = 0;
        std::vector<uint8_t> hbuf;
        auto rd = [&](void* dst, size_t n) {
            while (hbuf.size() < consumed + n) {
                if (hb_next >= z.blocks.size()) return false;
                const size_t at = hbuf.size();
                hbuf.resize(at + z.blocks[hb_next].isize);
                std::vector<size_t> off(1, 0);
                if (!z.inflate_blocks(hb_next, hb_next + 1, hbuf.data() + at, 0, &off).empty()) return false;
                hb_next++;
            }
            memcpy(dst, hbuf.data() + consumed, n);
            consumed += n;
            return true;
        };
        if (const char* e = parse_bam_header(rd, z.inflated_total(), S->hdr)) { S->err = *e ? e : "truncated BAM header"; return S; }
        size_t acc = 0;
        for (size_t k = 0; k < z.blocks.size(); k++) {
            if (consumed < acc + z.blocks[k].isize) { S->first_block = k; S->first_skip = consumed - acc; break; }
            acc += z.blocks[k].isize;
            S->first_block = k + 1; S->first_skip = 0;
        }
        S->have_bai = index.complete && index.ranges.size() == S->hdr.refs.size();
        if (S->have_bai) S->ref_range = std::move(index.ranges);
    } catch (const std::exception& e) { S->err = std::string("BAM header: ") + e.what(); }
    return S;
}

const char* bam_stream_error(void* h) { return ((BamStream*)h)->err.c_str(); }
const char* bam_stream_header_text(void* h) { return ((BamStream*)h)->hdr.text.c_str(); }
int64_t bam_stream_n_ref(void* h) { return (int64_t)((BamStream*)h)->hdr.refs.size(); }
const char* bam_stream_ref_name(void* h, int64_t i) { return ((BamStream*)h)->hdr.refs[(size_t)i].name.c_str(); }
int64_t bam_stream_ref_len(void* h, int64_t i) { return ((BamStream*)h)->hdr.refs[(size_t)i].length; }
int bam_stream_indexed(void* h) { return ((BamStream*)h)->have_bai ? 1 : 0; }
int64_t bam_stream_scan_parts(void* h) { return (int64_t)((BamStream*)h)->z.scan_parts; }
int64_t bam_stream_inflated_bytes(void* h) { return ((BamStream*)h)->inflated_bytes; }
int bam_stream_unique_names(void* h) { return ((BamStream*)h)->unique ? 1 : 0; }
int64_t bam_stream_head(void) { return (int64_t)BAM_STREAM_HEAD; }
void bam_stream_close(void* h) {
    BamStream* S = (BamStream*)h;
    if (S->inflating.valid()) (void)S->inflating.get();
    if (S->z.env.profile)
        fprintf(stderr, "stream profile (s): inflate %.3f in %lld windows, hop + names %.3f (threads %d)\n", S->t_inflate,
                (long long)S->n_windows, S->t_hop, S->z.threads);
    S->z.close();
    delete S;
}

// Restricts the stream to one contig.  *inflated_bound = inflated bytes of the blocks that will be read (an upper
// bound of the contig's record bytes when the file is indexed, of everything from the first record on otherwise).
int bam_stream_select(void* h, int32_t ref_id, int64_t* inflated_bound) {
    BamStream* S = (BamStream*)h;
    if (ref_id < 0 || (size_t)ref_id >= S->hdr.refs.size()) { S->err = "no such contig"; return 1; }
    if (S->inflating.valid()) (void)S->inflating.get();
    S->ready = false;
    S->target = ref_id; S->carry.clear(); S->names.clear(); S->nkept = 0; S->done = false; S->unique = true;
    S->kept_names.clear(); S->names_kept = S->keep_names;
    const auto& B = S->z.blocks;
    S->blk = S->first_block; S->skip = S->first_skip; S->blk_end = B.size();
    if (S->have_bai) {
        const auto rg = S->ref_range[(size_t)ref_id];
        if (rg.first == ~0ull) { S->blk = S->blk_end = 0; S->done = true; }       // no records on this contig
        else {
            auto find = [&](uint64_t foff) { size_t lo = 0, hi = B.size(); while (lo < hi) { const size_t m = (lo + hi) / 2; if (B[m].file_off < foff) lo = m + 1; else hi = m; } return lo; };
            const size_t b0 = find(rg.first >> 16), b1 = find(rg.second >> 16);
            if (b0 >= B.size() || B[b0].file_off != (rg.first >> 16)) { S->err = "index does not match the BAM file"; return 1; }
            S->blk = b0; S->skip = (size_t)(rg.first & 0xffff);
            S->blk_end = std::min(B.size(), b1 + 1);
        }
    }
    int64_t tot = 0;
    for (size_t k = S->blk; k < S->blk_end; k++) tot += B[k].isize;
    if (inflated_bound) *inflated_bound = tot;
    return 0;
}

// on != 0: the next bam_stream_select / pump also keeps the kept records' names by ordinal (off by default: the name
// table alone, no second copy).  bam_stream_read_name: the name of kept record `ordinal` of the selected contig, valid
// until the next select or close; null when that select kept no names or there is no such record.
void bam_stream_keep_names(void* h, int on) { ((BamStream*)h)->keep_names = on != 0; }
const char* bam_stream_read_name(void* h, int64_t ordinal) {
    BamStream* S = (BamStream*)h;
    if (!S->names_kept || ordinal < 0 || (size_t)ordinal >= S->kept_names.size()) return nullptr;
    return S->kept_names[(size_t)ordinal].c_str();
}

// Which bytes the pump sums for the device's text array: 0 the auxiliary fields (they hold the cs tag), 1 the
// CIGAR words (himut_ingest_derive_cs).  Exact either way, so no legal record outgrows what the host announced.
void bam_stream_sum_cigar(void* h, int on) { ((BamStream*)h)->cigar_sums = on != 0; }

// The whole loop of one contig's ingest in one call (no interpreter between the steps: a Python thread that parses the
// side VCFs meanwhile would otherwise hold the GIL against every one of them).  ``wait_fn`` / ``window_fn`` are
// libhimut_hip.so's himut_ingest_wait / himut_ingest_window, ``buf0`` / ``buf1`` its two pinned windows of ``cap`` bytes.
// Returns 0, -2 on a stream error (bam_stream_error), or the positive error code of the device library.
int bam_stream_pump(void* h, void* ctx, void* wait_fn, void* window_fn, uint8_t* buf0, uint8_t* buf1, int64_t cap, int64_t rec_cap) {
    BamStream* S = (BamStream*)h;
    int rc = -2;
    try { rc = pump_run(S, ctx, (ingest_wait_fn)wait_fn, (ingest_window_fn)window_fn, buf0, buf1, cap, rec_cap); }
    catch (const std::exception& e) { S->err = std::string("BAM stream: ") + e.what(); }
    // a failed pump may leave the next window's inflate running in the pool: it writes into the caller's buffers, which
    // the caller gives back to the process once it has the error, so the inflate is joined first
    if (rc != 0 && S->inflating.valid()) {
        try { (void)S->inflating.get(); } catch (const std::exception&) {}
    }
    return rc;
}

}  // extern "C"
