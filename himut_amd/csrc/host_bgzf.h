// BGZF for the host library (own implementation over zlib; no htslib): the reader that the whole-file loader
// (bam_load.cpp) and the streaming ingest (bam_stream.cpp) share, the writer of bam_write.cpp, and the HIMUT_INGEST_*
// switches that both readers honour.  Everything here is internal to libhimut_host.so.
#pragma once
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <string>
#include <thread>
#include <vector>

namespace {    // internal linkage in every source that includes this: the library exports its C functions only

inline uint32_t le32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint16_t le16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The HIMUT_INGEST_* switches (INTEGRATION.md lists them).  Read once per bam_load_threads / bam_stream_open call, on
// the calling thread, and carried by the Bgzf of that call: a later open sees a changed environment, and no worker
// thread reads the environment.
struct IngestEnv {
    int threads = 0;                            // HIMUT_INGEST_THREADS; 0: not set
    size_t window = (size_t)64 << 20;           // HIMUT_INGEST_WINDOW_KB: inflated bytes of a loader window (tests use small ones)
    size_t scan_min = (size_t)8 << 20;          // HIMUT_INGEST_SCAN_MIN_KB: below it the serial block scan is as fast (tests lower it)
    bool force_zlib = false;                    // HIMUT_INGEST_ZLIB: zlib's inflate even where libdeflate is found
    bool force_mmap = false;                    // HIMUT_INGEST_MMAP: compressed bytes through the mapping, not pread
    bool no_index = false;                      // HIMUT_INGEST_NO_INDEX: the stream ignores the .bai beside the file
    bool profile = false;                       // HIMUT_INGEST_PROFILE: seconds per stage on stderr
    IngestEnv() {
        if (const char* e = getenv("HIMUT_INGEST_THREADS")) threads = atoi(e);
        if (const char* e = getenv("HIMUT_INGEST_WINDOW_KB")) { const long kb = atol(e); if (kb > 0) window = (size_t)kb << 10; }
        if (const char* e = getenv("HIMUT_INGEST_SCAN_MIN_KB")) scan_min = (size_t)atol(e) << 10;
        force_zlib = getenv("HIMUT_INGEST_ZLIB") != nullptr;
        force_mmap = getenv("HIMUT_INGEST_MMAP") != nullptr;
        no_index = getenv("HIMUT_INGEST_NO_INDEX") != nullptr;
        profile = getenv("HIMUT_INGEST_PROFILE") != nullptr;
    }
    // threads of a call that names none: the variable, else one per hardware thread, at most `cap`
    int default_threads(unsigned cap) const {
        return threads > 0 ? threads : (int)std::min(cap, std::max(1u, std::thread::hardware_concurrency()));
    }
};

// BGZF reader: the file is mapped, its block headers are walked once (no inflate), and
// the blocks are inflated a window (~64 MB of output) at a time by a pool of threads --
// BGZF blocks are independent deflate streams.  The window after the one being parsed is
// inflated in the background, so record parsing and inflate overlap.
// libdeflate (about twice as fast as zlib's inflate) is used when the shared library is on the
// system; its three entry points are looked up at run time, zlib is the fallback.
struct Deflate {
    void* (*alloc)() = nullptr;
    int (*run)(void*, const void*, size_t, void*, size_t, size_t*) = nullptr;
    void (*release)(void*) = nullptr;
    Deflate() {
        void* h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        alloc = (void* (*)())dlsym(h, "libdeflate_alloc_decompressor");
        run = (int (*)(void*, const void*, size_t, void*, size_t, size_t*))dlsym(h, "libdeflate_deflate_decompress");
        release = (void (*)(void*))dlsym(h, "libdeflate_free_decompressor");
        if (!alloc || !run || !release) { alloc = nullptr; run = nullptr; release = nullptr; }
    }
    bool ok() const { return run != nullptr; }
};
inline const Deflate& deflate_lib() { static Deflate d; return d; }

struct BlockRef {
    size_t file_off;      // first byte of the block in the file (virtual file offsets of the index point here)
    size_t cdata_off;     // first byte of the deflate stream
    uint32_t cdata_len;
    uint32_t isize;       // inflated size
    size_t uoff;          // offset inside its window
};

struct Bgzf {
    const uint8_t* base = nullptr;   // mapped file
    size_t fsize = 0;
    int fd = -1;
    std::vector<uint8_t> owned;      // fallback when mmap is not possible
    std::vector<BlockRef> blocks;
    std::vector<size_t> win_first;   // first block of every window, + one past the end
    int threads = 1;
    IngestEnv env;
    std::string err;
    bool eof = false;

    std::vector<uint8_t> buf[2];     // two windows: one being parsed, one being inflated
    size_t cur = 0;                  // window being parsed
    size_t pos = 0, len = 0;
    std::future<std::string> pending;
    bool started = false;
    double t_first = 0, t_wait = 0;  // seconds inflating the first window / waiting for a later one (profile)

    size_t scan_parts = 1;           // stretches the block table was made from (threads used)

    bool open(const char* path, int nthreads, const IngestEnv& e, const std::vector<size_t>* hints = nullptr) {
        threads = nthreads < 1 ? 1 : nthreads;
        env = e;
        fd = ::open(path, O_RDONLY);
        if (fd < 0) { err = std::string("cannot open ") + path; return false; }
        struct stat st;
        if (fstat(fd, &st) != 0) { err = "fstat failed"; return false; }
        fsize = (size_t)st.st_size;
        if (fsize == 0) { err = "not a BAM file"; return false; }
        void* m = mmap(nullptr, fsize, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m != MAP_FAILED) {
            base = (const uint8_t*)m;
            (void)madvise(m, fsize, MADV_SEQUENTIAL);
        } else {
            owned.resize(fsize);
            size_t got = 0;
            while (got < fsize) {
                const ssize_t k = ::read(fd, owned.data() + got, fsize - got);
                if (k <= 0) { err = "read failed"; return false; }
                got += (size_t)k;
            }
            base = owned.data();
        }
        return scan(hints);
    }
    void close() {
        if (pending.valid()) (void)pending.get();
        if (base && owned.empty()) munmap((void*)base, fsize);
        if (fd >= 0) ::close(fd);
        base = nullptr; fd = -1;
    }
    // Block headers of the file range [p0, p1) -> (offset, compressed length, inflated length).  One pread per block:
    // the last four bytes of a block (its inflated length) and the header of the next block are neighbours.  (Through
    // the mapping a page fault per block costs several times more, and the pages are faulted in by the inflate threads
    // in parallel anyway.)  Returns "" or an error; "split" when the range does not end on a block boundary.
    std::string scan_range(size_t p0, size_t p1, std::vector<BlockRef>& out) const {
        uint8_t cur[64], nx[68];
        const bool pr = fd >= 0 && owned.empty();
        auto fetch = [&](size_t at, uint8_t* dst, size_t want) {
            const size_t w = std::min(want, fsize - at);
            if (!(pr && ::pread(fd, dst, w, (off_t)at) == (ssize_t)w)) memcpy(dst, base + at, w);
            return w;
        };
        size_t p = p0;
        if (p < p1) (void)fetch(p, cur, sizeof(cur));
        while (p < p1) {
            if (p + 18 > fsize) return "truncated BGZF header";
            const uint8_t* h = cur;
            if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) return "not a BGZF block";
            const unsigned xlen = le16(h + 10);
            if (p + 12 + xlen > fsize) return "truncated BGZF header";
            if (12 + xlen > sizeof(cur)) h = base + p;          // unusually long extra field: through the mapping
            int bsize = -1;
            for (size_t k = 0; k + 4 <= xlen;) {      // BC is normally the first subfield; tolerate others
                const uint8_t* e = h + 12 + k;
                const unsigned slen = le16(e + 2);
                if (e[0] == 'B' && e[1] == 'C' && slen == 2 && k + 6 <= xlen) bsize = le16(e + 4);
                k += 4 + slen;
            }
            if (bsize < 0) return "BGZF block without BC field";
            const size_t total = (size_t)bsize + 1;
            if (total < 12 + xlen + 8 || p + total > fsize) return "truncated BGZF block";
            const size_t got = fetch(p + total - 4, nx, sizeof(nx));
            out.push_back({p, p + 12 + xlen, (uint32_t)(total - 12 - xlen - 8), le32(nx), 0});
            p += total;
            memset(cur, 0, sizeof(cur));
            if (got > 4) memcpy(cur, nx + 4, got - 4);
        }
        return p == p1 ? "" : "split";
    }
    // The whole file's block table; windows of ~env.window output bytes.  ``hints``: file offsets at which blocks are
    // known to start (an index beside the file lists some): the table is then made by several threads, a stretch of the
    // file each; a hint that turns out wrong only costs the serial scan.
    bool scan(const std::vector<size_t>* hints = nullptr) {
        std::vector<size_t> cut(1, 0);
        const size_t T = (size_t)std::min(threads, 16);
        if (hints && !hints->empty() && T > 1 && fsize > env.scan_min)
            for (size_t i = 1; i < T; i++) {
                auto it = std::lower_bound(hints->begin(), hints->end(), fsize / T * i);
                if (it != hints->end() && *it > cut.back() && *it < fsize) cut.push_back(*it);
            }
        cut.push_back(fsize);
        const size_t np = cut.size() - 1;
        scan_parts = np;
        std::vector<std::vector<BlockRef>> part(np);
        std::vector<std::string> perr(np);
        if (np > 1) {
            std::vector<std::thread> pool;
            for (size_t i = 1; i < np; i++) pool.emplace_back([&, i]() { perr[i] = scan_range(cut[i], cut[i + 1], part[i]); });
            perr[0] = scan_range(cut[0], cut[1], part[0]);
            for (auto& th : pool) th.join();
            bool ok = true;
            for (const auto& e : perr) ok = ok && e.empty();
            if (!ok) { part.assign(1, {}); perr.assign(1, ""); cut = {0, fsize}; scan_parts = 1; }
        }
        if (part.size() == 1 && part[0].empty()) perr[0] = scan_range(0, fsize, part[0]);
        if (!perr[0].empty()) { err = perr[0] == "split" ? "truncated BGZF block" : perr[0]; return false; }
        size_t nb = 0;
        for (const auto& v : part) nb += v.size();
        blocks.reserve(nb);
        for (const auto& v : part) blocks.insert(blocks.end(), v.begin(), v.end());
        size_t wbytes = 0;
        win_first.push_back(0);
        for (size_t k = 0; k < blocks.size(); k++) {
            BlockRef& b = blocks[k];
            if (wbytes && wbytes + b.isize > env.window) { win_first.push_back(k); wbytes = 0; }
            b.uoff = wbytes;
            wbytes += b.isize;
        }
        win_first.push_back(blocks.size());
        return true;
    }
    size_t n_windows() const { return win_first.size() - 1; }
    // inflated bytes of the whole file: an upper bound for any size its header or a contig can claim
    size_t inflated_total() const { size_t n = 0; for (const BlockRef& b : blocks) n += b.isize; return n; }
    // inflates window w into out with the pool; returns an error text or ""
    std::string inflate_window(size_t w, std::vector<uint8_t>& out) const {
        const size_t b0 = win_first[w], b1 = win_first[w + 1];
        size_t total = 0;
        for (size_t k = b0; k < b1; k++) total += blocks[k].isize;
        out.resize(total);
        return inflate_blocks(b0, b1, out.data(), blocks[b0 < b1 ? b0 : 0].uoff);
    }
    // inflates blocks [b0, b1) with the pool: block k lands at dst + (uoff[k] - base_uoff) when the blocks belong to one
    // window, or back to back from dst when ``packed`` (any range)
    std::string inflate_blocks(size_t b0, size_t b1, uint8_t* dst, size_t base_uoff, const std::vector<size_t>* packed_off = nullptr) const {
        std::atomic<size_t> next(b0);
        std::atomic<int> bad(0);
        const bool use_pread = fd >= 0 && owned.empty() && !env.force_mmap;
        auto work = [&]() {
            const Deflate& L = deflate_lib();
            void* dec = (L.ok() && !env.force_zlib) ? L.alloc() : nullptr;
            z_stream zs;
            memset(&zs, 0, sizeof(zs));
            if (!dec && inflateInit2(&zs, -15) != Z_OK) { bad = 1; return; }
            // The compressed bytes are taken with pread into a buffer of the thread's own: through the shared mapping every
            // first touch of a page is a fault that takes the address space's lock, and the pool's threads queue up on it.
            std::vector<uint8_t> cbuf;
            if (use_pread) cbuf.resize(1 << 16);
            for (;;) {
                const size_t k = next.fetch_add(1);
                if (k >= b1) break;
                const BlockRef& b = blocks[k];
                if (!b.isize) continue;
                uint8_t* to = packed_off ? dst + (*packed_off)[k - b0] : dst + (b.uoff - base_uoff);
                const uint8_t* cin = base + b.cdata_off;
                if (use_pread && b.cdata_len <= cbuf.size() && ::pread(fd, cbuf.data(), b.cdata_len, (off_t)b.cdata_off) == (ssize_t)b.cdata_len)
                    cin = cbuf.data();
                if (dec) {
                    size_t got = 0;
                    if (L.run(dec, cin, b.cdata_len, to, b.isize, &got) != 0 || got != b.isize) { bad = 2; break; }
                } else {
                    inflateReset(&zs);
                    zs.next_in = (Bytef*)cin; zs.avail_in = b.cdata_len;
                    zs.next_out = to; zs.avail_out = b.isize;
                    if (inflate(&zs, Z_FINISH) != Z_STREAM_END) { bad = 2; break; }
                }
            }
            if (dec) L.release(dec); else inflateEnd(&zs);
        };
        const int nt = (int)std::min<size_t>((size_t)threads, b1 - b0 ? b1 - b0 : 1);
        std::vector<std::thread> pool;
        for (int t = 1; t < nt; t++) pool.emplace_back(work);
        work();
        for (auto& th : pool) th.join();
        return bad == 0 ? "" : (bad == 1 ? "inflateInit2 failed" : "inflate failed");
    }
    bool next_window() {
        if (!started) {
            started = true;
            if (n_windows() == 0) { eof = true; return false; }
            const double t0 = now_s();
            const std::string e = inflate_window(0, buf[0]);
            t_first += now_s() - t0;
            if (!e.empty()) { err = e; return false; }
            cur = 0;
        } else {
            if (cur + 1 >= n_windows()) { eof = true; return false; }
            const double t0 = now_s();
            const std::string e = pending.get();
            t_wait += now_s() - t0;
            if (!e.empty()) { err = e; return false; }
            cur++;
        }
        if (cur + 1 < n_windows()) {
            const size_t w = cur + 1;
            pending = std::async(std::launch::async, [this, w]() { return inflate_window(w, buf[w & 1]); });
        }
        pos = 0; len = buf[cur & 1].size();
        return true;
    }
    // n bytes of the stream without a copy when they lie inside the current window (scratch otherwise)
    const uint8_t* view(size_t n, std::vector<uint8_t>& scratch) {
        if (pos == len && !next_window()) return nullptr;
        if (len - pos >= n) { const uint8_t* p = buf[cur & 1].data() + pos; pos += n; return p; }
        scratch.resize(n);
        return read(scratch.data(), n) ? scratch.data() : nullptr;
    }
    bool read(void* dst, size_t n) {
        uint8_t* d = (uint8_t*)dst;
        while (n) {
            if (pos == len) { if (!next_window()) return false; continue; }
            const size_t k = len - pos < n ? len - pos : n;
            memcpy(d, buf[cur & 1].data() + pos, k);
            d += k; pos += k; n -= k;
        }
        return true;
    }
};

struct BgzfWriter {
    FILE* f;
    std::vector<uint8_t> buf;
    bool ok = true;
    uint64_t foff = 0;      // bytes of finished blocks
    uint64_t voffset() const { return (foff << 16) | (uint64_t)buf.size(); }   // virtual file offset of the next byte
    void flush_block(const uint8_t* data, size_t n) {
        std::vector<uint8_t> comp(n + 1024);
        z_stream zs;
        memset(&zs, 0, sizeof(zs));
        deflateInit2(&zs, 1, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
        zs.next_in = (Bytef*)data; zs.avail_in = (uInt)n;
        zs.next_out = comp.data(); zs.avail_out = (uInt)comp.size();
        deflate(&zs, Z_FINISH);
        const size_t clen = zs.total_out;
        deflateEnd(&zs);
        const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), data, (uInt)n);
        const uint16_t bsize = (uint16_t)(clen + 25);
        uint8_t hdr[18] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, (uint8_t)(bsize & 255), (uint8_t)(bsize >> 8)};
        uint8_t tail[8];
        for (int k = 0; k < 4; k++) { tail[k] = (uint8_t)(crc >> (8 * k)); tail[4 + k] = (uint8_t)((uint32_t)n >> (8 * k)); }
        ok = ok && fwrite(hdr, 1, 18, f) == 18 && fwrite(comp.data(), 1, clen, f) == clen && fwrite(tail, 1, 8, f) == 8;
        foff += 18 + clen + 8;
    }
    void write(const void* p, size_t n) {
        const uint8_t* d = (const uint8_t*)p;
        while (n) {
            size_t k = 0xff00 - buf.size() < n ? 0xff00 - buf.size() : n;
            buf.insert(buf.end(), d, d + k);
            d += k; n -= k;
            if (buf.size() == 0xff00) { flush_block(buf.data(), buf.size()); buf.clear(); }
        }
    }
    void finish() {
        if (!buf.empty()) { flush_block(buf.data(), buf.size()); buf.clear(); }
        flush_block(nullptr, 0);  // EOF marker block
    }
};

}  // namespace
