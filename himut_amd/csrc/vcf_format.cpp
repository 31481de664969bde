#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

// ---- VCF body text from the device's integer records ---------------------------------------
// What caller.records_to_tuples + vcflib._body_line print (reference: bamlib.py:181-219, caller.py:174-192,
// vcflib.py:820-1021), in C: the divisions are the same IEEE doubles and "%.1f" / "%.0f" / "%.2f" round
// like python's format (both print the correctly rounded decimal).  One 64-byte himut_record per entry
// (include/himut_hip.h).  sm_file = 1 writes only the rows of the single_molecule_mutations file.
// Returns the number of bytes written, or -1 if `cap` is too small.
struct VcfRec {
    int32_t tpos, chunk, phase_set, gq;
    uint8_t ref, alt, gt0, gt1, status, gt_state, flags, pad;
    uint32_t counts[6], bqsum[4];
};

static bool vcf_format_slice(const void* records, int64_t k0, int64_t k1, const char* chrom, int phased, int sm_file, std::string& out) {
    static const char* STATUS[] = {"PASS", "LowBQ", "LowGQ", "IndelSite", "HetSite", "HetAltSite", "HomAltSite", "ComSnp",
                                   "PanelOfNormal", "LowDepth", "HighDepth", "Unphased"};
    auto idx = [](int ch) { return ch == 'A' ? 0 : ch == 'T' ? 1 : ch == 'G' ? 2 : 3; };
    const VcfRec* R = (const VcfRec*)records;
    for (int64_t k = k0; k < k1; k++) {
        const VcfRec& r = R[k];
        const uint32_t* c = r.counts;
        const double depth = (double)(c[0] + c[1] + c[2] + c[3] + c[5]);
        const double ref_count = (double)c[idx(r.ref)];
        const bool hetalt = r.status == 5;
        char ps[16];
        if (r.phase_set >= 0) snprintf(ps, sizeof(ps), "%d", r.phase_set); else snprintf(ps, sizeof(ps), ".");
        char line[512];
        int m;
        if (hetalt) {
            const int pi = idx(r.gt0), qi = idx(r.gt1);
            const double pc = (double)c[pi], qc = (double)c[qi];
            if ((int64_t)ref_count != 1 && sm_file) continue;
            const char* fmt = (phased && sm_file) ? "GT:GQ:BQ:DP:AD:VAF:PS" : "GT:GQ:BQ:DP:AD:VAF";
            m = snprintf(line, sizeof(line), "%s\t%d\t.\t%c\t%c,%c\t.\t%s\t.\t%s\t./.:%d:%.1f,%.1f:%.0f:%.0f,%.0f,%.0f:%.2f,%.2f",
                         chrom, r.tpos, r.ref, r.gt0, r.gt1, STATUS[r.status], fmt, r.gq, (double)r.bqsum[pi] / pc,
                         (double)r.bqsum[qi] / qc, depth, ref_count, pc, qc, pc / depth, qc / depth);
        } else {
            const int ai = idx(r.alt);
            const double alt_count = (double)c[ai];
            if ((int64_t)alt_count != 1 && sm_file) continue;
            const double alt_bq = alt_count != 0 ? (double)r.bqsum[ai] / alt_count : 0.0;
            const char* fmt = phased ? "GT:GQ:BQ:DP:AD:VAF:PS" : "GT:GQ:BQ:DP:AD:VAF";
            m = snprintf(line, sizeof(line), "%s\t%d\t.\t%c\t%c\t.\t%s\t.\t%s\t./.:%d:%.1f:%.0f:%.0f,%.0f:%.2f", chrom, r.tpos,
                         r.ref, r.alt, r.status < 12 ? STATUS[r.status] : "?", fmt, r.gq, alt_bq, depth, ref_count, alt_count,
                         alt_count / depth);
        }
        if (m < 0 || m >= (int)sizeof(line) - 24) return false;
        out.append(line, (size_t)m);
        if (phased) { out.push_back(':'); out.append(ps); }
        out.push_back('\n');
    }
    return true;
}

// VCF body lines of n records into out (cap bytes); returns the length, or -1 when cap is too small.  Large inputs
// are formatted by a few threads, a slice of the records each, and the slices are laid end to end.
extern "C" int64_t vcf_format_records(const void* records, int64_t n, const char* chrom, int phased, int sm_file, char* out, int64_t cap) {
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)32, n / 8000, (int64_t)std::thread::hardware_concurrency()}));
    std::vector<std::string> part((size_t)nt);
    std::vector<char> ok((size_t)nt, 1);
    auto work = [&](int t) {
        part[(size_t)t].reserve((size_t)((n / nt + 1) * 64));
        ok[(size_t)t] = vcf_format_slice(records, n * t / nt, n * (t + 1) / nt, chrom, phased, sm_file, part[(size_t)t]) ? 1 : 0;
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; t++) pool.emplace_back(work, t);
    work(0);
    for (auto& th : pool) th.join();
    int64_t w = 0;
    for (int t = 0; t < nt; t++) {
        if (!ok[(size_t)t] || w + (int64_t)part[(size_t)t].size() > cap) return -1;
        memcpy(out + w, part[(size_t)t].data(), part[(size_t)t].size());
        w += (int64_t)part[(size_t)t].size();
    }
    return w;
}
