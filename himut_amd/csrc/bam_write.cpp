// Writes read batches out as BAM with its index (synthetic inputs for end-to-end runs and round-trip tests).
#include <map>

#include "host_bgzf.h"

static void w32(std::vector<uint8_t>& v, uint32_t x) { for (int k = 0; k < 4; k++) v.push_back((uint8_t)(x >> (8 * k))); }

// ---- writer: one call per file; contigs given as parallel arrays of batches -------------
struct BamWriteContig {
    const char* name;
    int64_t length;
    int64_t n;
    const int32_t *tstart, *qstart, *qlen;
    const uint8_t* mapq;
    const uint16_t* flag;
    const int32_t* qid;
    const int64_t *qoff, *cs_off;
    const uint8_t *seq, *bq, *cs, *tp;
    const uint8_t* names;        // the reads' names one behind the other, or null: read r is "ccs/<qid[r]>"
    const int64_t* name_off;     // n + 1 offsets into names
};

extern "C" int bam_write(const char* path, const char* sample, const BamWriteContig* contigs, int64_t n_contigs) {
    FILE* f = fopen(path, "wb");
    if (!f) return 1;
    BgzfWriter w{f, {}};
    std::string text = "@HD\tVN:1.6\tSO:coordinate\n";
    for (int64_t i = 0; i < n_contigs; i++)
        text += "@SQ\tSN:" + std::string(contigs[i].name) + "\tLN:" + std::to_string(contigs[i].length) + "\n";
    text += "@RG\tID:1\tSM:" + std::string(sample) + "\n";
    std::vector<uint8_t> hdr;
    hdr.insert(hdr.end(), {'B', 'A', 'M', 1});
    w32(hdr, (uint32_t)text.size());
    hdr.insert(hdr.end(), text.begin(), text.end());
    w32(hdr, (uint32_t)n_contigs);
    for (int64_t i = 0; i < n_contigs; i++) {
        const std::string nm = contigs[i].name;
        w32(hdr, (uint32_t)nm.size() + 1);
        hdr.insert(hdr.end(), nm.begin(), nm.end());
        hdr.push_back(0);
        w32(hdr, (uint32_t)contigs[i].length);
    }
    w.write(hdr.data(), hdr.size());
    std::vector<uint8_t> rec;
    std::vector<uint32_t> cigar;
    // index (.bai, SAM spec section 5.2): per contig the bins with their chunks and the 16-kb linear index
    struct RefIndex { std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins; std::vector<uint64_t> lin; uint64_t beg = 0, end = 0, n = 0; };
    std::vector<RefIndex> index((size_t)n_contigs);
    auto reg2bin = [](int64_t beg, int64_t end) -> uint32_t {
        --end;
        if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
        if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
        if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
        if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
        if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
        return 0;
    };
    for (int64_t ci = 0; ci < n_contigs; ci++) {
        const BamWriteContig& C = contigs[ci];
        for (int64_t r = 0; r < C.n; r++) {
            // CIGAR from the cs tag: S (clip) then M / I / D
            cigar.clear();
            const uint8_t* cs = C.cs + C.cs_off[r];
            const int64_t cn = C.cs_off[r + 1] - C.cs_off[r];
            int64_t qcons = C.qstart[r];
            if (C.qstart[r] > 0) cigar.push_back(((uint32_t)C.qstart[r] << 4) | 4);
            auto push = [&](uint32_t op, uint32_t ln) {
                if (!ln) return;
                if (!cigar.empty() && (cigar.back() & 15) == op) cigar.back() += ln << 4;
                else cigar.push_back((ln << 4) | op);
            };
            for (int64_t i = 0; i < cn;) {
                const char c = (char)cs[i];
                int64_t j = i + 1;
                if (c == ':') { uint32_t v = 0; while (j < cn && cs[j] >= '0' && cs[j] <= '9') v = v * 10 + (cs[j++] - '0'); push(0, v); qcons += v; }
                else if (c == '*') { j = i + 3; push(0, 1); qcons += 1; }
                else { while (j < cn && ((cs[j] | 32) >= 'a' && (cs[j] | 32) <= 'z')) j++; const uint32_t ln = (uint32_t)(j - i - 1);
                       if (c == '=') { push(0, ln); qcons += ln; } else if (c == '+') { push(1, ln); qcons += ln; } else push(2, ln); }
                i = j;
            }
            if (C.qlen[r] > qcons) cigar.push_back(((uint32_t)(C.qlen[r] - qcons) << 4) | 4);
            const std::string qname = C.names ? std::string((const char*)C.names + C.name_off[r], (size_t)(C.name_off[r + 1] - C.name_off[r]))
                                              : "ccs/" + std::to_string((long long)C.qid[r]);
            if (qname.empty() || qname.size() > 254) { fclose(f); return 3; }
            const uint32_t l_seq = (uint32_t)C.qlen[r];
            rec.clear();
            w32(rec, 0);  // block_size, patched below
            w32(rec, (uint32_t)ci);
            w32(rec, (uint32_t)C.tstart[r]);
            rec.push_back((uint8_t)(qname.size() + 1));
            rec.push_back(C.mapq[r]);
            rec.push_back(0x48); rec.push_back(0x12);  // bin (unused by this reader)
            rec.push_back((uint8_t)(cigar.size() & 255)); rec.push_back((uint8_t)(cigar.size() >> 8));
            rec.push_back((uint8_t)(C.flag[r] & 255)); rec.push_back((uint8_t)(C.flag[r] >> 8));
            w32(rec, l_seq);
            w32(rec, 0xffffffffu); w32(rec, 0xffffffffu); w32(rec, 0);
            rec.insert(rec.end(), qname.begin(), qname.end());
            rec.push_back(0);
            for (uint32_t c : cigar) w32(rec, c);
            const uint8_t* sq = C.seq + C.qoff[r] / 2;
            rec.insert(rec.end(), sq, sq + (l_seq + 1) / 2);
            const uint8_t* bq = C.bq + C.qoff[r];
            rec.insert(rec.end(), bq, bq + l_seq);
            rec.insert(rec.end(), {'c', 's', 'Z'});
            rec.insert(rec.end(), cs, cs + cn);
            rec.push_back(0);
            if (C.tp[r]) { rec.insert(rec.end(), {'t', 'p', 'A'}); rec.push_back(C.tp[r]); }
            const uint32_t bs = (uint32_t)rec.size() - 4;
            for (int k = 0; k < 4; k++) rec[k] = (uint8_t)(bs >> (8 * k));
            int64_t ref_len = 0;
            for (uint32_t c : cigar) if ((c & 15) == 0 || (c & 15) == 2) ref_len += c >> 4;
            const uint64_t v0 = w.voffset();
            w.write(rec.data(), rec.size());
            const uint64_t v1 = w.voffset();
            RefIndex& X = index[(size_t)ci];
            const int64_t beg = C.tstart[r], end = beg + (ref_len > 0 ? ref_len : 1);
            auto& ch = X.bins[reg2bin(beg, end)];
            if (!ch.empty() && ch.back().second == v0) ch.back().second = v1; else ch.emplace_back(v0, v1);
            for (int64_t wdw = beg >> 14; wdw <= (end - 1) >> 14; wdw++) {
                if ((size_t)wdw >= X.lin.size()) X.lin.resize((size_t)wdw + 1, 0);
                if (!X.lin[(size_t)wdw]) X.lin[(size_t)wdw] = v0;
            }
            if (!X.n) X.beg = v0;
            X.end = v1; X.n++;
        }
    }
    w.finish();
    bool ok = w.ok;
    fclose(f);
    if (ok) {
        std::vector<uint8_t> bai = {'B', 'A', 'I', 1};
        auto w64 = [&](uint64_t x) { for (int k = 0; k < 8; k++) bai.push_back((uint8_t)(x >> (8 * k))); };
        w32(bai, (uint32_t)n_contigs);
        for (auto& X : index) {
            w32(bai, (uint32_t)X.bins.size() + (X.n ? 1u : 0u));
            for (auto& kv : X.bins) {
                w32(bai, kv.first); w32(bai, (uint32_t)kv.second.size());
                for (auto& c : kv.second) { w64(c.first); w64(c.second); }
            }
            if (X.n) { w32(bai, 37450u); w32(bai, 2u); w64(X.beg); w64(X.end); w64(X.n); w64(0); }   // samtools' metadata pseudo-bin
            for (size_t k = 1; k < X.lin.size(); k++) if (!X.lin[k]) X.lin[k] = X.lin[k - 1];
            w32(bai, (uint32_t)X.lin.size());
            for (uint64_t v : X.lin) w64(v);
        }
        FILE* g = fopen((std::string(path) + ".bai").c_str(), "wb");
        ok = g && fwrite(bai.data(), 1, bai.size(), g) == bai.size();
        if (g) fclose(g);
    }
    return ok ? 0 : 2;
}
