// Host-side BAM ingest for the himut hot path (own implementation over zlib; no htslib).
//
// Reads a coordinate-sorted BAM (BGZF) sequentially and builds, per reference
// sequence, the structure-of-arrays read batch that himut_push_reads() takes
// (himut_amd/readbatch.py): what `pysam.AlignmentFile.fetch` + `bamlib.BAM` deliver to the
// reference worker (src/himut/bamlib.py:14-32, caller.py:299-300).
//
// Record fields kept: reference_start, reference_end (from CIGAR), leading soft clip
// (query_alignment_start), query length, MAPQ, FLAG, packed SEQ and QUAL as stored in the
// BAM, the cs:Z and tp:A tags, and the index of the first read with the same name.
#include <functional>
#include <unordered_map>

#include "host_bam.h"

namespace {

// growable byte buffer that does not zero what it grows by
// A contig's big arrays.  The copy pass that fills them is bound by first-touch page faults, so the arrays live in
// one anonymous mapping reserved up front (address space only: MAP_NORESERVE) and backed by huge pages where the
// kernel hands them out; growing inside the reservation costs nothing.  Without a reservation (or past it) the
// buffer grows by realloc / mremap.
struct RawBuf {
    uint8_t* p = nullptr;
    size_t n = 0, cap = 0;
    bool mapped = false;
    RawBuf() = default;
    RawBuf(const RawBuf&) = delete;
    RawBuf& operator=(const RawBuf&) = delete;
    RawBuf(RawBuf&& o) noexcept : p(o.p), n(o.n), cap(o.cap), mapped(o.mapped) { o.p = nullptr; o.n = o.cap = 0; o.mapped = false; }
    ~RawBuf() { if (mapped) munmap(p, cap); else free(p); }
    void reserve(size_t bytes) {
        if (p || bytes < ((size_t)8 << 20)) return;
        bytes = (bytes + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
        void* m = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (m == MAP_FAILED) return;
        (void)madvise(m, bytes, MADV_HUGEPAGE);
        p = (uint8_t*)m; cap = bytes; mapped = true;
    }
    bool grow(size_t want) {
        if (want > cap) {
            size_t nc = cap ? cap : 4096;
            while (nc < want) nc += nc / 2 + 4096;
            if (mapped) {
                void* q = mremap(p, cap, nc, MREMAP_MAYMOVE);
                if (q == MAP_FAILED) return false;
                p = (uint8_t*)q; cap = nc;
            } else {
                uint8_t* q = (uint8_t*)realloc(p, nc);
                if (!q) return false;
                p = q; cap = nc;
            }
        }
        n = want;
        return true;
    }
    const uint8_t* data() const { return p; }
    size_t size() const { return n; }
};

struct Contig {
    std::vector<int32_t> tstart, tend, qstart, qlen, qid;
    std::vector<uint8_t> mapq, tp;
    std::vector<uint16_t> flag;
    std::vector<int64_t> qoff, cs_off;
    RawBuf seq, bq, cs;
    std::unordered_map<std::string, int32_t> first_by_name;
    int64_t bases_padded = 0, cs_n = 0;
};

struct Bam {
    BamHeader hdr;
    std::string err;
    std::vector<Contig> contigs;            // one per hdr.refs entry
    int64_t n_missing_cs = 0, n_unmapped = 0, n_unsorted = 0;
};

// walks the auxiliary fields; returns false on a malformed block
bool scan_tags(const uint8_t* p, const uint8_t* end, const uint8_t** cs, size_t* cs_len, uint8_t* tp) {
    *cs = nullptr; *cs_len = 0; *tp = 0;
    while (p + 3 <= end) {
        const char t0 = (char)p[0], t1 = (char)p[1], ty = (char)p[2];
        p += 3;
        size_t sz = 0;
        switch (ty) {
            case 'A': case 'c': case 'C': sz = 1; break;
            case 's': case 'S': sz = 2; break;
            case 'i': case 'I': case 'f': sz = 4; break;
            case 'Z': case 'H': {
                const uint8_t* q = p;
                while (q < end && *q) q++;
                if (q >= end) return false;
                if (t0 == 'c' && t1 == 's' && ty == 'Z') { *cs = p; *cs_len = (size_t)(q - p); }
                p = q + 1;
                continue;
            }
            case 'B': {
                if (p + 5 > end) return false;
                const char sub = (char)p[0];
                const uint32_t cnt = le32(p + 1);
                const uint64_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
                if ((uint64_t)(end - p) < 5 + es * (uint64_t)cnt) return false;     // the array runs past the record
                p += 5 + es * cnt;
                continue;
            }
            default: return false;
        }
        if (p + sz > end) return false;
        if (t0 == 't' && t1 == 'p' && ty == 'A') *tp = p[0];
        p += sz;
    }
    return true;
}

void* load(Bam* B, const char* path, int threads) {
    const IngestEnv env;
    Bgzf z;
    if (threads <= 0) threads = env.default_threads(16);
    if (!z.open(path, threads, env)) { B->err = z.err; z.close(); return B; }
    auto fail = [&](const std::string& m) { B->err = m.empty() ? "unexpected end of BAM" : m; z.close(); return (void*)B; };
    const size_t inflated_total = z.inflated_total();       // an upper bound for any size the header claims, any contig's bytes
    if (const char* e = parse_bam_header([&](void* dst, size_t n) { return z.read(dst, n); }, inflated_total, B->hdr))
        return fail(z.err.empty() ? e : z.err);
    const uint32_t n_ref = (uint32_t)B->hdr.refs.size();
    B->contigs.resize(n_ref);
    // Records are parsed a window at a time: the record boundaries of the window are found by hopping from
    // length field to length field, the records are decoded by the pool (CIGAR walk, tag scan), a short
    // sequential pass assigns every kept record its place in its contig's arrays, and the pool copies the bytes.
    struct RecInfo {
        const uint8_t* rec; uint32_t bs;
        int32_t ref_id, pos, lead_clip; int64_t ref_len;
        uint32_t l_seq, cs_len; uint16_t flag; uint8_t mapq, tp, l_qname, status;   // status: 0 keep, 1 unmapped, 2 no cs
        const uint8_t *seq, *qual, *cs; const char* qname;
        int64_t dst_bases, dst_cs; Contig* C;
    };
    struct { double hop = 0, decode = 0, place = 0, grow = 0, copy = 0; } prof;      // seconds per stage (env.profile)
    std::string perr;
    auto decode = [&](RecInfo& I) -> bool {
        const uint8_t* rec = I.rec;
        const uint32_t bs = I.bs;
        I.ref_id = (int32_t)le32(&rec[0]);
        I.pos = (int32_t)le32(&rec[4]);
        I.l_qname = rec[8];
        I.mapq = rec[9];
        const uint16_t n_cigar = le16(&rec[12]);
        I.flag = le16(&rec[14]);
        I.l_seq = le32(&rec[16]);
        I.status = 0;
        if (I.ref_id < 0 || (uint32_t)I.ref_id >= n_ref || (I.flag & 4)) { I.status = 1; return true; }
        if (!record_fits(rec, bs)) return false;
        size_t o = 32;
        I.qname = (const char*)&rec[o];
        o += I.l_qname;
        int64_t ref_len = 0;
        int32_t lead_clip = 0;
        bool seen_query = false;
        for (uint16_t k = 0; k < n_cigar; k++) {
            const uint32_t c = le32(&rec[o + 4 * k]);
            const uint32_t op = c & 15, ln = c >> 4;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += ln;   // M D N = X
            if (op == 4 && !seen_query) lead_clip += (int32_t)ln;                   // leading S
            if (op == 0 || op == 1 || op == 7 || op == 8) seen_query = true;        // M I = X
        }
        I.ref_len = ref_len; I.lead_clip = lead_clip;
        o += 4ull * n_cigar;
        I.seq = &rec[o];
        o += (I.l_seq + 1) / 2;
        I.qual = &rec[o];
        o += I.l_seq;
        size_t cs_len = 0;
        if (!scan_tags(&rec[o], rec + bs, &I.cs, &cs_len, &I.tp)) return false;
        I.cs_len = (uint32_t)cs_len;
        if (!I.cs) I.status = 2;
        return true;
    };
    auto place = [&](RecInfo& I) {          // sequential: order matters
        if (I.status == 1) { B->n_unmapped++; return; }
        if (I.status == 2) { B->n_missing_cs++; return; }
        Contig& C = B->contigs[(size_t)I.ref_id];
        if (!C.tstart.empty() && I.pos < C.tstart.back()) B->n_unsorted++;
        if (C.tstart.empty()) {             // first record of the contig: reserve address space for its arrays
            const size_t bound = std::min<size_t>(2 * inflated_total, (size_t)48 << 30);
            C.bq.reserve(bound); C.seq.reserve(bound / 2); C.cs.reserve(std::min<size_t>(inflated_total, (size_t)16 << 30));
        }
        const int32_t idx = (int32_t)C.tstart.size();
        C.tstart.push_back(I.pos);
        C.tend.push_back((int32_t)(I.pos + I.ref_len));
        C.qstart.push_back(I.lead_clip);
        C.qlen.push_back((int32_t)I.l_seq);
        C.mapq.push_back(I.mapq);
        C.flag.push_back(I.flag);
        C.tp.push_back(I.tp);
        auto it = C.first_by_name.emplace(std::string(I.qname, strnlen(I.qname, I.l_qname)), idx);
        C.qid.push_back(it.first->second);
        C.qoff.push_back(C.bases_padded);
        I.C = &C; I.dst_bases = C.bases_padded; I.dst_cs = C.cs_n;
        C.bases_padded += ((int64_t)I.l_seq + 31) & ~(int64_t)31;
        C.cs_off.push_back(C.cs_n);
        C.cs_n += I.cs_len;
    };
    auto copy_bytes = [&](const RecInfo& I) {
        if (I.status) return;
        Contig& C = *I.C;
        const int64_t padded = ((int64_t)I.l_seq + 31) & ~(int64_t)31;
        uint8_t* sq = C.seq.p + I.dst_bases / 2;
        const size_t nsq = (I.l_seq + 1) / 2;
        memcpy(sq, I.seq, nsq);
        if (I.l_seq & 1) sq[nsq - 1] &= 0xf0;
        memset(sq + nsq, 0, (size_t)(padded / 2) - nsq);               // pad to the 32-base boundary
        uint8_t* bq = C.bq.p + I.dst_bases;
        memcpy(bq, I.qual, I.l_seq);
        memset(bq + I.l_seq, 0, (size_t)padded - I.l_seq);
        if (I.cs_len) memcpy(C.cs.p + I.dst_cs, I.cs, I.cs_len);
    };
    auto run_pool = [&](size_t count, const std::function<void(size_t)>& f) {
        const int nt = (int)std::min<size_t>((size_t)z.threads, count / 64 + 1);
        if (nt <= 1) { for (size_t k = 0; k < count; k++) f(k); return; }
        std::atomic<size_t> next(0);
        auto work = [&]() { for (;;) { const size_t k0 = next.fetch_add(64); if (k0 >= count) break; for (size_t k = k0; k < std::min(count, k0 + 64); k++) f(k); } };
        std::vector<std::thread> pool;
        for (int t = 1; t < nt; t++) pool.emplace_back(work);
        work();
        for (auto& th : pool) th.join();
    };
    auto finish_batch = [&](std::vector<RecInfo>& recs) -> bool {
        std::atomic<int> bad(0);
        double t0 = now_s();
        run_pool(recs.size(), [&](size_t k) { if (!decode(recs[k])) bad = 1; });
        prof.decode += now_s() - t0;
        if (bad) { perr = "malformed BAM record"; return false; }
        t0 = now_s();
        for (auto& I : recs) place(I);
        prof.place += now_s() - t0;
        t0 = now_s();
        for (auto& C : B->contigs)
            if (!C.seq.grow((size_t)(C.bases_padded / 2)) || !C.bq.grow((size_t)C.bases_padded) || !C.cs.grow((size_t)C.cs_n)) {
                perr = "out of memory"; return false;
            }
        prof.grow += now_s() - t0;
        t0 = now_s();
        run_pool(recs.size(), [&](size_t k) { copy_bytes(recs[k]); });
        prof.copy += now_s() - t0;
        recs.clear();
        return true;
    };
    std::vector<uint8_t> scratch;
    std::vector<RecInfo> recs;
    auto list = [&](const uint8_t* rec, uint32_t bs) {
        RecInfo I;
        memset(&I, 0, sizeof(I));
        I.rec = rec; I.bs = bs;
        recs.push_back(I);
        return true;
    };
    uint8_t b4[4];
    for (;;) {
        // whole records inside the current window
        if (z.pos == z.len && !z.next_window()) { if (z.eof && z.err.empty()) break; return fail(z.err); }
        const double t_hop = now_s();
        if (const char* e = hop_records(z.buf[z.cur & 1].data(), z.pos, z.len, list)) return fail(e);
        prof.hop += now_s() - t_hop;
        if (!finish_batch(recs)) return fail(perr);
        if (z.pos == z.len) continue;
        // a record that runs into the next window: assembled in scratch, handled on its own
        if (!z.read(b4, 4)) { if (z.eof && z.err.empty()) break; return fail(z.err); }
        const uint32_t bs = le32(b4);
        if (const char* e = record_length_error(bs)) return fail(e);
        const uint8_t* rec = z.view(bs, scratch);
        if (!rec) return fail(z.err.empty() ? "truncated BAM record" : z.err);
        list(rec, bs);
        if (!finish_batch(recs)) return fail(perr);
    }
    for (auto& C : B->contigs) { C.cs_off.push_back(C.cs_n); C.first_by_name.clear(); }
    z.close();
    if (env.profile)
        fprintf(stderr, "ingest profile (s): first window %.3f, waiting for inflate %.3f, hop %.3f, decode %.3f, place %.3f, "
                        "grow %.3f, copy %.3f (threads %d)\n", z.t_first, z.t_wait, prof.hop, prof.decode, prof.place, prof.grow,
                prof.copy, threads);
    return B;
}

}  // namespace

extern "C" {

// Loads the whole file with `threads` inflate threads (0: HIMUT_INGEST_THREADS, else one per hardware thread, at most
// 16).  Returns a handle (never null); check bam_error().
void* bam_load_threads(const char* path, int threads) {
    Bam* B = new Bam();
    try {
        return load(B, path, threads);
    } catch (const std::exception& e) {         // e.g. bad_alloc / length_error on a corrupt header: an error, not an abort
        B->err = std::string("BAM load failed: ") + e.what();
        return B;
    }
}

const char* bam_error(void* h) { return ((Bam*)h)->err.c_str(); }
const char* bam_header_text(void* h) { return ((Bam*)h)->hdr.text.c_str(); }
int64_t bam_n_ref(void* h) { return (int64_t)((Bam*)h)->hdr.refs.size(); }
const char* bam_ref_name(void* h, int64_t i) { return ((Bam*)h)->hdr.refs[(size_t)i].name.c_str(); }
int64_t bam_ref_len(void* h, int64_t i) { return ((Bam*)h)->hdr.refs[(size_t)i].length; }
int64_t bam_ref_nreads(void* h, int64_t i) { return (int64_t)((Bam*)h)->contigs[(size_t)i].tstart.size(); }
int64_t bam_ref_bases_padded(void* h, int64_t i) { return ((Bam*)h)->contigs[(size_t)i].bases_padded; }
int64_t bam_ref_cs_bytes(void* h, int64_t i) { return (int64_t)((Bam*)h)->contigs[(size_t)i].cs.size(); }
int64_t bam_count(void* h, int what) {
    Bam* B = (Bam*)h;
    return what == 0 ? B->n_missing_cs : what == 1 ? B->n_unmapped : B->n_unsorted;
}

// the per-read arrays of a contig, copied out (the three big ones: bam_ref_bytes)
void bam_ref_copy(void* h, int64_t i, int32_t* tstart, int32_t* tend, int32_t* qstart, int32_t* qlen, uint8_t* mapq,
                  uint16_t* flag, int32_t* qid, int64_t* qoff, int64_t* cs_off, uint8_t* tp) {
    const Contig& C = ((Bam*)h)->contigs[(size_t)i];
    const size_t n = C.tstart.size();
    auto cp = [](void* d, const void* s, size_t b) { if (b) memcpy(d, s, b); };
    cp(tstart, C.tstart.data(), n * 4); cp(tend, C.tend.data(), n * 4); cp(qstart, C.qstart.data(), n * 4);
    cp(qlen, C.qlen.data(), n * 4); cp(mapq, C.mapq.data(), n); cp(flag, C.flag.data(), n * 2);
    cp(qid, C.qid.data(), n * 4); cp(qoff, C.qoff.data(), n * 8); cp(cs_off, C.cs_off.data(), (n + 1) * 8);
    cp(tp, C.tp.data(), n);
}

// the three big arrays of a contig in place (valid until bam_free): 0 seq, 1 bq, 2 cs
const uint8_t* bam_ref_bytes(void* h, int64_t i, int which) {
    const Contig& C = ((Bam*)h)->contigs[(size_t)i];
    return which == 0 ? C.seq.data() : which == 1 ? C.bq.data() : C.cs.data();
}

void bam_free(void* h) { delete (Bam*)h; }

}  // extern "C"
