// What the whole-file loader (bam_load.cpp) and the streaming ingest (bam_stream.cpp) both know about the BAM layout
// (SAM specification, section 4.2): the header, the size checks of a record, the hop from length field to length field.
// The per-record helpers are inline on purpose: they sit in the hop loops of both.
#pragma once
#include "host_bgzf.h"

namespace {    // internal linkage in every source that includes this: the library exports its C functions only

struct BamHeader {
    struct Ref { std::string name; int64_t length = 0; };
    std::string text;
    std::vector<Ref> refs;
};

// Reads the header through ``read(dst, n)`` (false when the stream has no n more bytes).  ``inflated_total``: the bytes
// the whole file inflates to; a length the header claims is checked against it before anything of that size is
// allocated.  Returns nullptr, or why the header is refused: "" when the stream ended inside it, which the caller words.
template <class Read>
const char* parse_bam_header(Read&& read, size_t inflated_total, BamHeader& H) {
    uint8_t b4[4];
    if (!read(b4, 4) || memcmp(b4, "BAM\1", 4) != 0) return "not a BAM file";
    if (!read(b4, 4)) return "";
    const uint32_t l_text = le32(b4);
    if ((size_t)l_text > inflated_total) return "BAM header text longer than the file";
    H.text.resize(l_text);
    if (l_text && !read(&H.text[0], l_text)) return "";
    while (!H.text.empty() && H.text.back() == '\0') H.text.pop_back();
    if (!read(b4, 4)) return "";
    const uint32_t n_ref = le32(b4);
    if ((size_t)n_ref * 8 > inflated_total) return "BAM header lists more contigs than the file can hold";
    H.refs.resize(n_ref);
    for (BamHeader::Ref& R : H.refs) {
        if (!read(b4, 4)) return "";
        const uint32_t l_name = le32(b4);
        if ((size_t)l_name > inflated_total) return "contig name longer than the file";
        R.name.assign(l_name, '\0');
        if (l_name && !read(&R.name[0], l_name)) return "";
        while (!R.name.empty() && R.name.back() == '\0') R.name.pop_back();
        if (!read(b4, 4)) return "";
        R.length = le32(b4);
    }
    return nullptr;
}

// ---- one record: ``rec`` is its body, behind the length field ``bs`` (block_size) ----
inline const char* record_length_error(uint32_t bs) { return bs < 32 ? "BAM record too short" : nullptr; }

// the fixed part, the name, the CIGAR, SEQ and QUAL: what stands in front of the auxiliary fields
inline uint64_t record_fixed_bytes(const uint8_t* rec) {
    const uint64_t l_qname = rec[8], n_cigar = le16(rec + 12), l_seq = le32(rec + 16);
    return 32 + l_qname + 4 * n_cigar + (l_seq + 1) / 2 + l_seq;
}
inline bool record_fits(const uint8_t* rec, uint32_t bs) { return record_fixed_bytes(rec) <= bs; }

// Steps over the whole records of buf[pos, len): take(rec, bs) per record, which returns false to stop in front of
// it.  ``pos`` ends at the first byte not stepped over: a record the buffer cuts, or the one take() refused.
// Returns nullptr, or the error text of a length field no record can have.
template <class Take>
const char* hop_records(const uint8_t* buf, size_t& pos, size_t len, Take&& take) {
    while (pos + 4 <= len) {
        const uint32_t bs = le32(buf + pos);
        if (const char* e = record_length_error(bs)) return e;
        if (pos + 4 + (size_t)bs > len) break;
        if (!take(buf + pos + 4, bs)) break;
        pos += 4 + (size_t)bs;
    }
    return nullptr;
}

}  // namespace
