/*
 * himut_hip.h -- C ABI of libhimut_hip.so: the MI355X (gfx950) implementation of
 * himut's per-chromosome CCS pileup scan.
 *
 * The reference (sjin09/himut v1.0.4) has no plugin/FFI interface; its only seam
 * for this path is the Python worker
 *     himut.caller.get_somatic_substitutions      src/himut/caller.py:208-642
 * called once per contig by Pool.starmap (caller.py:805-808).  One himut_ctx
 * stands for one such worker bound to one GPU; the entry points below are what a
 * binding of that worker needs (INTEGRATION.md shows the ctypes stub):
 *
 *   worker argument / step (reference)                  entry point
 *   --------------------------------------------------  -------------------------
 *   16 scalar thresholds        caller.py:217-236       himut_set_params
 *   gtlib.init + log10 tables   gtlib.py:12-20,47-69    himut_set_gt_lut
 *   chunkloci_lst               caller.py:213,268       himut_set_chunks
 *   pon_sbs_set/common_snp_set  caller.py:245-262       himut_set_site_set
 *   phase_set2{hbit,hpos,hetsnp} caller.py:214-216      himut_set_phase
 *   alignments.fetch + BAM()    caller.py:299-300,
 *                               bamlib.py:14-32         himut_push_reads
 *   the body of the worker      caller.py:264-621       himut_run
 *   chrom2tsbs_lst[chrom]       caller.py:622-624       himut_get_records
 *   chrom2tsbs_log[chrom]       caller.py:625-641       himut_get_log
 *
 * Conventions: plain pointers and sizes only.  The caller owns every input
 * buffer and may free it when the call returns.  The library owns device
 * memory and the buffers returned by himut_get_records until the next
 * himut_run / himut_destroy.  Every function returns 0 on success or a
 * HIMUT_ERR_* code; himut_last_error() gives the message.  No C++ exception
 * crosses the boundary.  A context is single-threaded; contexts are independent
 * (one per GPU, driven by one host thread or process each).
 */
#ifndef HIMUT_HIP_H
#define HIMUT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIMUT_ABI_VERSION 2

typedef struct himut_ctx himut_ctx;

/* error codes (return values) */
enum {
    HIMUT_OK = 0,
    HIMUT_ERR_ARG = 1,          /* bad argument / call order */
    HIMUT_ERR_HIP = 2,          /* HIP runtime failure */
    HIMUT_ERR_CS = 3,           /* cs tag the reference's tokenizer (cslib.py:7-10) cannot split, or cs inconsistent
                                   with SEQ/CIGAR */
    HIMUT_ERR_BASE = 4,         /* KeyError in the reference: base outside ATGC (util.py:17) */
    HIMUT_ERR_BQ0 = 5,          /* ValueError in the reference: log10(0) for BQ 0 (gtlib.py:64) */
    HIMUT_ERR_CHUNK = 6,        /* chunk with start > end (pysam raises) */
    HIMUT_ERR_COVER = 7,        /* KeyError in tpos2qbase (haplib.py:51) */
    HIMUT_ERR_RESERVED8 = 8,    /* (never returned; kept so that the codes behind it do not move) */
    HIMUT_ERR_NOMEM = 9,
    HIMUT_ERR_DEPTH = 10        /* the contig's candidate columns need more than 2^32 column-store slots (or one
                                   256-position window holds more than 2^22 reads): split the contig's chunk list;
                                   himut_run_callable: a position with more than 65,535 callable read bases */
};

/* FILTER column values (caller.py:349-621, vcflib.py:189-209) */
enum {
    HIMUT_ST_PASS = 0, HIMUT_ST_LOWBQ = 1, HIMUT_ST_LOWGQ = 2, HIMUT_ST_INDEL = 3, HIMUT_ST_HET = 4,
    HIMUT_ST_HETALT = 5, HIMUT_ST_HOMALT = 6, HIMUT_ST_COMSNP = 7, HIMUT_ST_PON = 8, HIMUT_ST_LOWDEPTH = 9,
    HIMUT_ST_HIGHDEPTH = 10, HIMUT_ST_UNPHASED = 11,
    /* himut_run_sites only (no FILTER of the reference): the site is what is_germ_gt drops; no read covers the site */
    HIMUT_ST_GERMLINE = 12, HIMUT_ST_NOCOV = 13,
    /* himut_run_sindels only: the allele lengthens or shortens a homopolymer run of the reference longer than max_run */
    HIMUT_ST_REPEAT = 14
};

/* The scalar arguments of the worker (caller.py:217-236).  somatic_snv_prior and
 * germline_indel_prior are accepted by the reference but never read inside the
 * worker; germline_snv_prior enters through himut_set_gt_lut. */
typedef struct himut_params {
    int32_t min_qv;
    int32_t min_mapq;
    int32_t qlen_lower_limit;
    int32_t qlen_upper_limit;
    int32_t min_gq;
    int32_t min_bq;
    int32_t max_mismatch_count;
    int32_t mismatch_window_size;
    int32_t md_threshold;
    int32_t min_ref_count;
    int32_t min_alt_count;
    int32_t min_hap_count;
    int32_t phase;              /* 0 / 1 */
    int32_t reserved;
    double min_sequence_identity;
    double min_trim;
} himut_params;

/* The non-secondary alignments of one contig in BAM file order (coordinate
 * sorted).  Layout: himut_amd/readbatch.py.  seq is BAM 4-bit packed, bq raw
 * Phred, cs the concatenated cs:Z strings; qoff[i] (multiple of 32) is read i's
 * base offset into seq (in bases) and bq. */
typedef struct himut_read_batch {
    int64_t n_reads;
    const int32_t* tstart;      /* reference_start, 0-based */
    const int32_t* tend;        /* reference_end, exclusive (from CIGAR) */
    const int32_t* qstart;      /* query_alignment_start (leading soft clip) */
    const int32_t* qlen;        /* len(query_sequence) */
    const uint8_t* mapq;
    const uint16_t* flag;       /* SAM flag; 0x100 reads are skipped (bamlib.py:17) */
    const int32_t* qid;         /* index of the first read with the same query name */
    const int64_t* qoff;
    const int64_t* cs_off;      /* n_reads + 1 entries */
    const uint8_t* seq;
    const uint8_t* bq;
    const uint8_t* cs;
    int64_t seq_bytes;
    int64_t bq_bytes;
    int64_t cs_bytes;
} himut_read_batch;

/* One evaluated candidate, integers only: the host divides and formats exactly
 * as bamlib.py:181-219 / caller.py:174-192 / vcflib.py:820-1021 do. 64 bytes. */
typedef struct himut_record {
    int32_t tpos;               /* 1-based POS */
    int32_t chunk;              /* index of the chunk that evaluated it */
    int32_t phase_set;          /* chunk start for a phased PASS (caller.py:292,584), else -1 */
    int32_t gq;                 /* germ_gq (gtlib.py:138-174) */
    uint8_t ref, alt;           /* ASCII */
    uint8_t gt0, gt1;           /* germline genotype, reference allele first when het (gtlib.py:133-134) */
    uint8_t status;             /* HIMUT_ST_* */
    uint8_t gt_state;           /* 0 homref 1 het 2 hetalt 3 homalt */
    uint8_t flags;              /* internal; 0 in returned records */
    uint8_t pad;
    uint32_t counts[6];         /* A T G C ins del (util.py:14-20 order) at rpos = tpos - 1; ins = the reads with an insertion in
                                   front of the position (the reference counts insertion OPERATIONS, which is one more for a read
                                   whose cs holds two insertions in a row; nothing it prints depends on the number, only on != 0) */
    uint32_t bqsum[4];          /* sum of BQ per allele A T G C */
} himut_record;

/* Per-run figures for bench.py / DESIGN.md (times from hipEvents on the
 * context's stream, in milliseconds).  A stage time is 0 unless its events were
 * recorded: see himut_set_stage_timing. */
typedef struct himut_run_stats {
    double ms_total;
    double ms_parse;            /* k_parse_cs: cs decode, one wave per group of reads (+ k_window_index and the fills beside it) */
    double ms_bqsum;            /* 0: the quality sum is taken inside k_stream_capture (kept for ABI layout) */
    double ms_hap;              /* k_read_hap (phase only) */
    double ms_emit;             /* the candidate list from the mask the capture's proposals set.  Chunks in
                                   coordinate order: k_mask_emit alone (mask by column rank; + k_scan_small where
                                   the host sizes the records by the count first).  Any other chunk list:
                                   k_scan_small, k_mask_emit_cells and the sort */
    double ms_index;            /* k_mark_positions (bitmap of substitution positions) + rank, column windows /
                                   offsets, column-store fill: runs in front of the capture */
    double ms_capture;          /* k_stream_capture: streams every read once, fills the column store, sums the
                                   qualities of every read.  After himut_run_normcounts: k_norm_quad, the sweep's
                                   dominant kernel, by itself (ms_parse = the decode, ms_index = the read pass,
                                   ms_eval = the whole position sweep) */
    double ms_eval;             /* k_eval_columns: counts, ordered likelihood sums, genotype, filters */
    double ms_finalize;         /* cross-chunk som_seen / counters / compaction */
    int64_t n_reads;
    int64_t read_bases;         /* sum of qlen */
    int64_t positions;          /* sum over chunks of (end - start + 1) */
    int64_t n_unique_positions; /* reserved */
    int64_t n_candidates;       /* evaluated candidates before the cross-chunk pass */
    int64_t n_records;
    int64_t column_slots;       /* column-store slots (unique candidate positions x reads in their windows) */
    int64_t reran;              /* 1 when the run was repeated with exact buffer sizes because a count exceeded the
                                   capacities kept from the previous run: ms_* then describe the second pass only
                                   and the wall time of himut_run covers both */
} himut_run_stats;

int himut_abi_version(void);
int himut_create(int device, himut_ctx** out);
void himut_destroy(himut_ctx* ctx);
const char* himut_last_error(const himut_ctx* ctx);

int himut_set_params(himut_ctx* ctx, const himut_params* p);
/* three tables of n_bq doubles indexed by BQ, and log10 priors in the order
 * homref, het, hetalt, homalt */
int himut_set_gt_lut(himut_ctx* ctx, const double* log_hom, const double* log_het, const double* log_err, int n_bq,
                     const double log_prior[4]);
int himut_set_chunks(himut_ctx* ctx, const int32_t* start, const int32_t* end, int64_t n_chunks);
/* which: 0 panel of normals, 1 common SNPs.  keys sorted ascending:
 * (pos1 << 4) | (ref << 2) | alt with A0 T1 G2 C3. */
int himut_set_site_set(himut_ctx* ctx, int which, const uint64_t* keys, int64_t n);
/* per chunk c (phase set keyed str(chunk_start), caller.py:292-295): hetSNPs
 * off[c]..off[c+1] with 1-based hpos, ASCII ref/alt (0 when not a single base)
 * and hbit '0'/'1'. */
int himut_set_phase(himut_ctx* ctx, const int64_t* off, const int32_t* hpos, const uint8_t* href,
                    const uint8_t* halt, const uint8_t* hbit, int64_t n_chunks);
int himut_push_reads(himut_ctx* ctx, const himut_read_batch* batch);
int himut_run(himut_ctx* ctx);
/* himut_run in two halves, for a caller that scans several contigs (a context each): begin queues the whole run and --
 * on any run but a context's first on its reads and chunks -- returns without waiting; end waits for the run's last
 * copy, checks it and makes the results available.  Runs of different contexts begun one after the other share the GPU
 * without the host in between.  A context must not be touched between its begin and its end. */
int himut_run_begin(himut_ctx* ctx);
int himut_run_end(himut_ctx* ctx);
int himut_get_records(himut_ctx* ctx, const himut_record** records, int64_t* n);
int himut_get_log(himut_ctx* ctx, int64_t out[15]);
int himut_get_stats(himut_ctx* ctx, himut_run_stats* out);
/* Which hipEvents himut_run records (each costs a barrier packet, i.e. a few microseconds of queue time):
 * 0 = run start / end only (ms_total), 1 = also around k_stream_capture (ms_capture; the default),
 * 2 = every stage of himut_run_stats.  No counterpart in the reference (it has no timers). */
int himut_set_stage_timing(himut_ctx* ctx, int level);

/* Device-resident copy of the result for the multi-GPU gather: number of
 * records, and a device-to-device copy into caller-provided device memory
 * (e.g. a torch tensor handed to RCCL). */
int himut_records_device(himut_ctx* ctx, const void** dev_ptr, int64_t* n);
int himut_copy_records_to_device(himut_ctx* ctx, void* dst_device, int64_t capacity_records);

/* ---- next row: the BAM ingest in front of the path (reference call sites caller.py:267,299:
 * pysam.AlignmentFile + alignments.fetch, and the record wrapper bamlib.BAM.__init__, bamlib.py:14-32).
 * An alternative to himut_push_reads: the contig's inflated BAM records go to HBM a window at a time and are parsed
 * there (CIGAR walk, tag scan, placement, byte copies: csrc/himut_ingest.h).  The caller inflates BGZF blocks straight
 * into one of the library's two pinned buffers (himut_ingest_buffer), lists where the records of the contig start
 * (rec_off: offset of each record's body, i.e. behind its block_size field, from byte `start` of the buffer, where the
 * window's nbytes begin) and which earlier record carries the same
 * read name (qid, as in himut_read_batch), and hands the window over; the copy of window k overlaps the inflate of
 * window k + 1 (two buffers: himut_ingest_wait(slot) returns once slot's bytes have left the host).  padded_bases =
 * sum of the records' l_seq rounded up to 32, tag_bytes = an upper bound of the cs text in the window (the bytes of
 * the records' auxiliary fields): what the library must have room for.  himut_ingest_end leaves the context as
 * himut_push_reads would.  The two pinned buffers belong to the PROCESS (pinning them takes tens of milliseconds): one
 * ingest may be open at a time -- himut_ingest_begin on a second context before the first's himut_ingest_end (or
 * himut_destroy) returns HIMUT_ERR_ARG.  libhimut_host.so's bam_stream_* (csrc/bam_ingest.cpp) is the host side that goes with it. */
typedef struct himut_ingest_result {
    int64_t n_reads, bases_padded, cs_bytes, read_bases;
    int64_t n_missing_cs;       /* records without a cs tag (the reference's get_tag("cs") raises KeyError, bamlib.py:32) */
    int64_t n_unsorted;         /* records in front of their predecessor: not coordinate sorted */
    int64_t n_malformed;
} himut_ingest_result;
int himut_ingest_begin(himut_ctx* ctx, int64_t inflated_bytes_bound, int64_t window_bytes);
void* himut_ingest_buffer(himut_ctx* ctx, int slot);
int himut_ingest_wait(himut_ctx* ctx, int slot);
int himut_ingest_window(himut_ctx* ctx, int slot, int64_t start, int64_t nbytes, const uint32_t* rec_off, const int32_t* qid,
                        int64_t n_rec, int64_t padded_bases, int64_t tag_bytes);
int himut_ingest_end(himut_ctx* ctx, int unique_qnames, himut_ingest_result* out);
/* Files without cs:Z (pbmm2 output, archived HiFi BAMs): the cs text is a function of CIGAR, SEQ and the reference bases
 * under the alignment, so the ingest can write it itself.  mode 0 (default): the records' cs:Z tags are the text, a
 * record without one is counted in n_missing_cs.  mode 1: the text of EVERY record is derived from its CIGAR and the
 * string given to himut_set_reference (short form; M, = and X alike, the bases decide; a cs tag that is present is
 * ignored), n_missing_cs is 0 and himut_ingest_result.cs_bytes counts the derived text.  The mode holds for every
 * himut_ingest_begin after the call, until it is set again; HIMUT_ERR_ARG if mode is 1 and no reference has been set.
 * A record is underivable -- counted, never guessed at -- with no CIGAR op, with an N or P op (the placeholder of a
 * CIGAR kept in CG:B has one), when its query-consuming ops do not add up to l_seq, or when it leaves the reference
 * string; himut_ingest_end then leaves the context without reads.  tag_bytes of himut_ingest_window is, in mode 1, a
 * bound of the window's CIGAR bytes (4 * n_cigar_op summed).
 * himut_ingest_derive_result, after himut_ingest_end: out[0] records derived, out[1] underivable records, out[2] bytes
 * of derived text, out[3] device milliseconds of the post-pass that wrote it. */
int himut_ingest_derive_cs(himut_ctx* ctx, int mode);
int himut_ingest_derive_result(himut_ctx* ctx, int64_t out[4]);
/* per-read fields the host needs for bamlib.get_thresholds (bamlib.py:137-178); any pointer may be null */
int himut_ingest_read_meta(himut_ctx* ctx, int32_t* tstart, int32_t* tend, int32_t* qlen, uint8_t* mapq, uint8_t* tp);
/* the resident read batch back on the host (arrays of the caller, sized by the fields of `batch` on entry) */
int himut_download_reads(himut_ctx* ctx, himut_read_batch* batch, uint8_t* tp);

/* ---- next row: normcounts.get_callable_tricounts ---------------------------------
 * The worker's arguments (normcounts.py:206-241) map onto the same calls as the call path
 * (params, LUT, chunks, site sets, phase sets, reads) plus the contig's reference string:
 *   seq (str(refseq[chrom]), normcounts.py:504)          himut_set_reference
 *   the body of the worker (normcounts.py:243-402)       himut_run_normcounts
 *   chrom2{ccs,ref}_callable_tri2count, chrom2norm_log   himut_get_normcounts
 * seq is passed as the FASTA holds it (case matters: the reference skips positions whose base
 * is not an upper-case A/C/G/T).  cls[256] maps every byte of seq to a class id < n_classes
 * (one class per distinct byte, A C G T N always present, at most 32); the two histograms
 * are indexed (c0 * K + c1) * K + c2 over the class ids of the trinucleotide key.
 * alt_order[ref * 3 + i] = allele of list(base_set.difference(ref))[i] (normcounts.py:367): the
 * order python gives that set decides PoN/common precedence and ties, so the host supplies it.
 * log[14] in the order of chrom2norm_log (normcounts.py:404-419). */
int himut_set_reference(himut_ctx* ctx, const uint8_t* seq, int64_t len, const uint8_t cls[256], int n_classes);
int himut_run_normcounts(himut_ctx* ctx, const uint8_t alt_order[12], int non_human_sample);
int himut_get_normcounts(himut_ctx* ctx, int64_t* ccs_tri, int64_t* ref_tri, int64_t log[14]);
/* Test hook, no counterpart in the reference: which sweep himut_run_normcounts takes (0: k_norm_quad with its two lists,
 * the default; 1: k_norm_tile for the whole contig; 2: as 0, but the host takes the first pass as if its list of tiles had been
 * too short, so that the contig is swept again by k_norm_tile), the capacity of one part of the list of positions left to
 * k_norm_dirty (0: sized from the contig) and how many of a wave's pool slots may be handed out (0: all) -- sweep 2 and
 * the last two make the fall-back paths run on small inputs.  Results never depend on any of them. */
int himut_debug_normcounts(himut_ctx* ctx, int sweep, int64_t dirty_list_cap, int pool_slots);
/* Test hook, no counterpart in the reference: the device bytes the context holds for himut_run_normcounts' sweep.
 * out[0]: the plan (items and their counts per tile), out[1]: the list of positions left to k_norm_dirty (entries, the
 * parts' counters and the layout table), out[2]: the list of tiles left to k_norm_tile, out[3]: their total. */
int himut_debug_norm_scratch(himut_ctx* ctx, int64_t out[4]);
/* Test hook, no counterpart in the reference: the bits k_callable wrote in the last pass, one per query base, and the
 * reads that passed the read filters.  Valid only after himut_run_normcounts has completed on the pushed batch
 * (HIMUT_ERR_ARG otherwise, and when n_words or n_reads exceeds what the pass wrote: bq_bytes / 32 words, n_reads bytes).
 * Waits for the context's stream, then copies the first n_words words and the first n_reads bytes.  Bit q & 31 of word
 * (qoff[r] + q) >> 5 is query base q of read r, q from offset 0 of the query (soft clip included).  Changes nothing. */
int himut_debug_norm_callable(himut_ctx* ctx, uint32_t* words, int64_t n_words, uint8_t* live, int64_t n_reads);
/* reflib.get_chrom_tricount (reflib.py:11-33) of the string given to himut_set_reference: out[first * 16 + centre * 4 +
 * last], letters A0 C1 G2 T3, purine centres already turned to the other strand (so 32 of the 64 bins fill).
 * himut_get_stats afterwards: ms_total = the device time of the kernel (the other fields stay as they were). */
int himut_ref_tricounts(himut_ctx* ctx, int64_t out[64]);
/* reflib.get_chrom_tricount of one FASTA record as the file holds it: body / n are the bytes of its sequence lines,
 * line ends included (host memory; an mmap of the file will do).  The sequence is what is left after deleting '\n',
 * '\r', '\t' and ' '; out[64] as himut_ref_tricounts.  The bytes go through the process's two pinned windows (the
 * ones the ingest uses): HIMUT_ERR_ARG while an ingest is open on them. */
int himut_fasta_tricounts(himut_ctx* ctx, const uint8_t* body, int64_t n, int64_t out[64]);
/* Test hook, no counterpart in the reference: the staging window of himut_fasta_tricounts in bytes (0: the default,
 * 64 MiB), so that small inputs put window ends inside whitespace runs.  Results never depend on it. */
int himut_debug_fasta_window(himut_ctx* ctx, int64_t window_bytes);

/* ---- next row: mutlib.load_sbs96_counts / get_sbs96 (mutlib.py:1998-2018, 2058-2102) of the contig whose
 * string was given to himut_set_reference.  pos0 / ref / alt: the PASS bi-allelic single-base substitutions of that
 * contig as the VCF holds them (0-based position, ASCII).  out[sub * 16 + up * 4 + down] for the 96 classes (sub in the
 * order C>A C>G C>T T>A T>C T>G, A0 C1 G2 T3, purine references read on the other strand); out[96] = classes that
 * contain an N (the reference drops them), out[97] = classes outside the 96 without an N (KeyError in the reference),
 * out[98] = position + 1 behind the string (IndexError in the reference). */
int himut_sbs96_counts(himut_ctx* ctx, const int32_t* pos0, const uint8_t* ref, const uint8_t* alt, int64_t n, int64_t out[99]);
/* mutlib.load_sbs1536_counts / get_sbs1536 (mutlib.py:2021-2055, 2105-2149): the same inputs, two letters of context a side.
 * out[sub * 256 + uu * 64 + u * 16 + d * 4 + dd] for the 1536 classes (sbs1536_lst order); out[1536] = classes that
 * contain an N, out[1537] = classes outside the 1536 without an N, out[1538] = position + 2 behind the string.  Reads
 * below position 0 wrap to the end of the string, as python's negative indices do. */
int himut_sbs1536_counts(himut_ctx* ctx, const int32_t* pos0, const uint8_t* ref, const uint8_t* alt, int64_t n, int64_t out[1539]);

/* ---- the indel and doublet spectra (no counterpart in the reference).  The 83 and 78 classes
 * are COSMIC's, in SigProfiler's order; the rules below that put an allele into a class are this package's definition.
 *
 * himut_id83_classify: n indel alleles of the contig whose string was given to himut_set_reference (seq, reflen letters).
 * Allele i is (anchor0[i] = a, 0-based; type[i]: 0 deletion, 1 insertion; len[i] = L in 1..64; bases + 16 * i: the inserted
 * bases, 2 bits a base with the codes of "ATGC", base j in bits 2 * (j & 3) of byte j >> 2 -- himut_indel_record's packing,
 * read for insertions only).  A deletion removes seq[a+1 .. a+L]; an insertion puts its bases I between seq[a] and seq[a+1].
 * Letters compare without case; a byte outside ACGTacgt matches nothing, itself included; nothing in front of seq[0] or
 * behind seq[reflen-1] is read (no wrap-around).  The allele's periodic extent is m = l + r with
 *   deletion   r = the largest k with seq[a+1+L+j] == seq[a+1+j] for all j < k,
 *              l = the largest k with seq[a-j] == seq[a+L-j] for all j < k;
 *   insertion  r = the largest k with seq[a+1+j] == I[j mod L] for all j < k,
 *              l = the largest k with seq[a-j] == I[(L-1-j) mod L] for all j < k (the index taken into 0..L-1),
 * the scan ending once m >= 5L (no class looks further: at most 320 comparisons an allele).  m is what shifting the allele
 * left as far as it goes, rotating an insertion's bases, and scanning right finds: the class does not depend on where
 * inside its repeat the allele was placed.  Classes, in bin order:
 *    0..11   1:Del:C:0..5, 1:Del:T:0..5   L = 1, deletion; the deleted letter, G as C and A as T; min(m, 5)
 *   12..23   1:Ins:C:0..5, 1:Ins:T:0..5   L = 1, insertion; the inserted letter likewise; min(m, 5)
 *   24..47   2:Del:R:0..5 .. 5:Del:R:0..5  L >= 2, deletion, m >= L or m == 0; size min(L, 5); min(m / L, 5)
 *   48..71   2:Ins:R:0..5 .. 5:Ins:R:0..5  L >= 2, insertion; size min(L, 5); min(m / L, 5)
 *   72..82   2:Del:M:1; 3:Del:M:1,2; 4:Del:M:1..3; 5:Del:M:1..5   L >= 2, deletion, 0 < m < L; size min(L, 5); min(m, 5)
 * out[83] = alleles whose deleted stretch holds a byte outside ACGTacgt, out[84] = alleles with a < 0, a + L >= reflen
 * (deletion) or a >= reflen (insertion); out[85..87] = 0, reserved.  cls (may be null): the class per allele, 255 for an
 * allele counted in out[83] or out[84].  Site sets, parameters, regions and reads are neither read nor changed.
 * himut_get_stats afterwards: ms_total = the device time of the kernel, ms_parse = the upload of the list in front of it.
 * HIMUT_ERR_ARG, with a message and the context usable as before: no reference string, n < 0, a null array with n > 0,
 * a length outside 1..64, a type above 1. */
int himut_id83_classify(himut_ctx* ctx, const int32_t* anchor0, const uint8_t* type, const int32_t* len, const uint8_t* bases,
                        int64_t n, uint8_t* cls, int64_t out[88]);
/* himut_dbs78_counts: n doublets, ref2 / alt2 two ASCII letters each (n x 2), either case.  If the reference pair is one of
 * AC AT CC CG CT GC TA TC TG TT the doublet is taken as it is, else reference and alternative are both reverse-
 * complemented; for AT, CG, GC and TA an alternative that is not listed is replaced by its reverse complement (COSMIC's
 * representatives).  The 78 bins, in order:
 *   AC> CA CG CT GA GG GT TA TG TT   AT> CA CC CG GA GC TA      CC> AA AG AT GA GG GT TA TG TT   CG> AT GC GT TA TC TT
 *   CT> AA AC AG GA GC GG TA TC TG   GC> AA AG AT CA CG TA      TA> AT CG CT GC GG GT
 *   TC> AA AG AT CA CG CT GA GG GT   TG> AA AC AT CA CC CT GA GC GT   TT> AA AC AG CA CC CG GA GC GG
 * out[78] = doublets with a letter outside ACGT, out[79] = doublets in which either base is unchanged; cls (may be null):
 * the class per doublet, 255 for one counted in out[78] or out[79].  Needs no reference string.  HIMUT_ERR_ARG for n < 0 or
 * a null array with n > 0. */
int himut_dbs78_counts(himut_ctx* ctx, const uint8_t* ref2, const uint8_t* alt2, int64_t n, uint8_t* cls, int64_t out[80]);
/* Test hook: the most workgroups k_id83 and k_dbs78 are launched with (0: the default, 2048), so that short lists make
 * the kernels stride; the three strand kernels below take the same cap.  Results never depend on it. */
int himut_debug_spectra(himut_ctx* ctx, int max_workgroups);

/* ---- signature exposures with bootstrap intervals (no counterpart in the reference).  The
 * definition is this package's.
 *
 * Inputs: integer counts m[c], c < C, N their sum; a non-negative matrix S[c][k] (sig, [C][K] row-major), k < K, whose
 * columns each sum to 1 -- normalising them is the caller's job, the library does not re-normalise.
 *
 * Fit: multiplicative EM for the Poisson / multinomial mixture, `iters` iterations, no early stop.
 *   start        e[k] = (double)N / (double)K for every k
 *   step 1       for every c: r[c] = sum over k of S[c][k] * e[k], summed sequentially in ascending k from 0.0;
 *                q[c] = (m[c] == 0 || r[c] == 0.0) ? 0.0 : (double)m[c] / r[c]
 *   step 2       for every k: g = sum over c of S[c][k] * q[c], summed sequentially in ascending c from 0.0;
 *                e[k] = e[k] * g
 * All arithmetic is IEEE fp64, one correctly rounded multiply and one correctly rounded add per term, nothing contracted,
 * subnormals kept.  These orders are the specification: the result is defined to the bit.
 *
 * Bootstrap: replicate 0 is m itself.  Replicate b (1 <= b <= n_boot) draws N mutations; draw i (0 <= i < N) takes
 *   z = seed + 0x9E3779B97F4A7C15 * (1 + b * 2^32 + i);  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *   z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31   (all mod 2^64);  j = ((z >> 32) * N) >> 32
 * and lands in the smallest c whose inclusive prefix sum of m exceeds j: a channel with m[c] == 0 is never drawn.  Each
 * replicate's counts are fitted as above, with the same N.
 *
 * exposures[(n_boot + 1)][K]: row b = e of replicate b.  resampled (may be null): [(n_boot + 1)][C], row b = the counts
 * of replicate b.  Limits: 1 <= C <= 1536, 1 <= K <= 96, 0 <= N < 2^31 and no negative count, 0 <= n_boot <= 100000,
 * 1 <= iters <= 100000, every sig entry finite and >= 0; anything else, or a null sig, counts or exposures, is
 * HIMUT_ERR_ARG with a message, before anything is queued and with the context usable as before.  The call reads nothing
 * else of the context -- no reads, reference, site sets, regions or parameters -- and changes none of them; it runs on
 * the context's stream in its scratch pools.  himut_get_stats afterwards: ms_total = the device time of the two kernels,
 * ms_hap = k_fit_resample, ms_eval = k_fit_em, ms_parse = the upload in front of them; n_candidates = n_boot + 1,
 * n_unique_positions = workgroups of k_fit_em, n_records = replicates per workgroup of k_fit_em, column_slots = that workgroup's LDS bytes, positions = those of them
 * that hold S (0: S is read from global memory). */
int himut_fit_exposures(himut_ctx* ctx, const double* sig, int32_t C, int32_t K, const int64_t* counts, int32_t n_boot,
                        uint64_t seed, int32_t iters, double* exposures, int32_t* resampled);
/* Test hook: the most workgroups k_fit_resample and k_fit_em are launched with (0: the default, 2048), so that a few
 * replicates make them stride, and the bytes of LDS a workgroup of k_fit_em may take (0: the default, 65536; at most
 * that), so that a small matrix takes the path that reads S from global memory.  S is held in LDS whenever it fits the
 * budget beside one replicate's arrays, with as many replicates (up to four) beside it as still fit; else up to four
 * replicates share a workgroup and S is read from global memory.  One replicate's own arrays are held in
 * LDS whatever the budget.  Results never depend on either. */
int himut_debug_fit(himut_ctx* ctx, int max_workgroups, int lds_budget_bytes);

/* ---- the transcription-strand spectrum, SBS384, and its opportunity counts (no counterpart
 * in the reference).  The definitions are this package's:
 *
 * Genes are stranded intervals on the contig whose string was given to himut_set_reference; the host hands them over as
 * a segment list.  seg_start[k] is ascending with seg_start[0] == 0; segment k covers [seg_start[k], seg_start[k + 1]),
 * the last one runs to the string's end.  seg_mask[k] is 0..3: bit 0 = some gene on '+' covers the segment, bit 1 = some
 * gene on '-' does.  Neighbouring segments may carry equal masks; a contig without genes is one segment of mask 0.
 *
 * The category of a position in a segment of mask m depends on whether the letter at the position -- the VCF's REF for a
 * substitution, the centre letter for a trinucleotide -- is a purine, that is, is read on the other strand by
 * himut_sbs96_counts / himut_ref_tricounts:
 *     mask 0          N (3) either way
 *     mask 1 ('+')    pyrimidine here: U (1)    purine here: T (0)
 *     mask 2 ('-')    pyrimidine here: T (0)    purine here: U (1)
 *     mask 3          B (2) either way
 * T: the pyrimidine of the pair lies on the transcribed (template) strand -- SigProfiler's convention.  Order T, U, B, N.
 *
 * SBS384 bin = category * 96 + k, k exactly the bin himut_sbs96_counts gives the substitution (letters, wrap-around and
 * the three flag counters as there); a flagged substitution has no category.  Label: T:A[C>A]A.
 * Trinucleotide class = first * 8 + (centre == T ? 4 : 0) + last after the fold (himut_run_intervals' numbering); it
 * exists only when all three letters are upper-case ACGT; no wrap-around, a position at either end has none.
 *
 * himut_set_strands: needs himut_set_reference first.  HIMUT_ERR_ARG, with a message and the context usable as before
 * (an earlier list stays), all checked on the host before anything is queued: n_seg < 1, seg_start[0] != 0, a start not
 * above its predecessor, a start >= reflen, a mask above 3.  A later himut_set_reference drops the list. */
int himut_set_strands(himut_ctx* ctx, const int32_t* seg_start, const uint8_t* seg_mask, int64_t n_seg);
/* The substitutions of himut_sbs96_counts (same arrays) by category: out[category * 96 + k], out[384..386] = the three
 * flags out[96..98] of himut_sbs96_counts.  cls (may be null): the bin per substitution, 0xFFFF for a flagged one.
 * HIMUT_ERR_ARG: no reference string, no segment list, n < 0, a null array with n > 0. */
int himut_sbs384_counts(himut_ctx* ctx, const int32_t* pos0, const uint8_t* ref, const uint8_t* alt, int64_t n, uint16_t* cls,
                        int64_t out[387]);
/* out[category * 32 + class] over the resident string: summed over the categories, the 32 bins himut_ref_tricounts fills.
 * HIMUT_ERR_ARG: no reference string, no segment list. */
int himut_strand_tricounts(himut_ctx* ctx, int64_t out[128]);
/* The same tally over the entries of the last completed himut_run_callable's map, CALLABLE entries only: an entry adds 1
 * to pos[category * 32 + class] and its callable bases to bases[...].  A position held by two chunks counts twice, as
 * everywhere else.  Summed over the categories: ref_tri[0..31] / ccs_tri[0..31] of himut_run_intervals for one interval
 * over the contig.  HIMUT_ERR_ARG: himut_run_intervals' preconditions (a completed callable run, a reference string as
 * long as the one it saw), no segment list.
 * After each of the three, himut_get_stats' ms_total is the device time of the kernel. */
int himut_strand_callable(himut_ctx* ctx, int64_t pos[128], int64_t bases[128]);

/* ---- next row: phaselib.get_edges (phaselib.py:16-67) --------------------------------
 * hpos / href: the contig's heterozygous SNPs (1-based position ascending, ASCII reference base), as
 * vcflib.load_hetsnps lists them.  For every primary read with mapq >= min_mapq and every ordered pair (i, j) of
 * the hetSNPs it spans whose base qualities are >= min_bq:  counts[(i * band + (j - i - 1)) * 4 + k] += 1 with
 * k = 0 cis1 (ref, ref), 1 cis2 (other, other), 2 trans1 (ref, other), 3 trans2 (other, ref).  band must be at least the
 * largest number of hetSNPs one read spans minus one (HIMUT_ERR_ARG otherwise).  A deleted position has quality 0 and a base
 * that is not the reference base: with min_bq <= 0 it counts, with state "other".  counts holds max(n_het, 1) * band * 4
 * entries; the slots that name no edge (i + 1 + d >= n_het) stay zero. */
int himut_run_edges(himut_ctx* ctx, const int32_t* hpos, const uint8_t* href, int64_t n_het, int min_bq, int min_mapq,
                    int64_t band, uint32_t* counts);

/* ---- germline SNVs from the call path's pile.  No counterpart in the reference, which takes the germline VCF of
 * `phase --vcf` (phaselib.py), `call --phase` and vcflib.get_germline_priors from an external caller; what is the reference's
 * is the pile (caller.py:44-72,299-305) and the genotyper (gtlib.get_germ_gt, gtlib.py:122-135).
 * Inputs: himut_set_gt_lut, himut_set_chunks (the regions: they select which positions are reported, they never shape
 * a pile), the reads.  himut_set_params is not needed and what it set is left alone.  The pile of a 0-based position:
 * every read that covers it with flag 0x100 clear and mapq >= min_mapq, in file order.  Candidates: the positions at
 * which a pile read carries a substitution and start <= tpos <= end holds for some region; each is genotyped once.
 * FILTER, first rule that holds (alt alleles = the genotype's alleles other than the reference base): LowGQ gq < min_gq;
 * LowBQ an alt allele without a read of bq >= min_bq; LowDepth an alt allele's count < min_alt_count, or het and the
 * reference allele's count < min_ref_count; HighDepth A+T+G+C+del > md_threshold (bamlib.get_read_depth); else PASS.
 * report_homref = 1: a homref candidate is a record too (gt_state 0, alt = ref, status PASS).
 * Records (himut_get_germline): ascending tpos, chunk = phase_set = -1, alt = the first alt allele, status one of the
 * HIMUT_ST_* codes above.  log[12]: positions genotyped, positions whose substitutions name n as the reference base
 * (skipped), homref, het, hetalt, homalt, PASS, LowGQ, LowBQ, LowDepth, HighDepth, 0 (the FILTER counters over the
 * non-homref positions).  HIMUT_ERR_ARG without tables, regions or reads; HIMUT_ERR_CS when reads disagree about a
 * position's reference base.  himut_get_records / himut_records_device keep serving the last call run. */
typedef struct himut_germline_params {
    int32_t min_mapq, min_gq, min_bq, min_ref_count, min_alt_count, md_threshold, report_homref, reserved;
} himut_germline_params;
int himut_run_germline(himut_ctx* ctx, const himut_germline_params* p);
int himut_get_germline(himut_ctx* ctx, const himut_record** records, int64_t* n, int64_t log[12]);

/* ---- the reads that carry each substitution of a site list.  No counterpart in the reference: its authors made such
 * tables with scripts outside the package (scripts/sbs2ccs.py, scripts/sbs_qpos_distribution.py); what is the reference's
 * is the substitution list (cslib.cs2subindel, cslib.py:47-64), the quality mean (bamlib.py:34-36) and the mismatch
 * window (bamlib.py:245-282).
 * Inputs: the reads, and n_sites sites (pos1, ref, alt): pos1 a 1-based VCF POS, non-decreasing; ref / alt ASCII upper-case
 * letters of ATGC, ref != alt.  Equal positions with different alleles and repeated triples are allowed, each site is
 * answered on its own; anything else is HIMUT_ERR_ARG.  himut_set_params, himut_set_gt_lut and himut_set_chunks are not
 * needed and what they set is left alone, as are the position bitmap, the candidate mask and the scalars of the call
 * and germline runs.  HIMUT_ERR_ARG without reads; n_sites == 0 is a run with zero rows.
 * Reads in play: flag 0x100 clear and mapq >= min_mapq (supplementary alignments are in); every alignment is a read of
 * its own, whatever its name.  A read covers a site iff tstart <= pos1 - 1 < tend; it supports a site iff its
 * substitution list (letters upper-cased, substitutions with reference base N left out) holds (pos1, ref, alt).  A site
 * whose ref disagrees with the reads' cs text has no supporting read; that is no error.  A quality 0 or a query base
 * outside ATGC raises nothing here; malformed cs text raises what the decode raises.
 * One row per (site, supporting read), ascending by (site, read); two runs on the same input give the same bytes.
 * window_mismatches: with (s, e) = bamlib.get_mismatch_range(pos1, qpos, qlen, mismatch_window_size), the entries of the
 * read's mismatch list (substitutions and indel operations) with s <= position <= e, minus one: the number
 * bamlib.is_mismatch_conflict compares with max_mismatch_count.
 * himut_get_support: rows and site_counts (n_sites x {cover, alt_reads}) are the library's, valid until the next
 * himut_run_support or himut_destroy; himut_get_records and himut_get_germline keep serving their own last runs.
 * himut_get_stats after the run: ms_total, ms_parse (stage timing 2), n_reads, read_bases, n_records = rows. */
typedef struct himut_support_row {
    int32_t site;               /* index into the site arrays */
    int32_t read;               /* ordinal of the read in the batch = file order */
    int32_t qid;                /* as in himut_read_batch */
    int32_t tstart, tend, qlen; /* the read's */
    uint16_t flag;              /* the read's SAM flag */
    uint8_t mapq;
    uint8_t bq;                 /* the quality at qpos */
    int32_t qpos;               /* query offset of the substitution as cs2subindel's qsbs_lst holds it: leading soft clip included */
    uint32_t bq_sum;            /* sum of the read's qlen qualities: bq_sum / qlen is BAM.get_qv */
    int32_t n_sub;              /* entries of the read's tsbs_lst */
    int32_t n_indel;            /* insertion plus deletion operations: len(mismatch_lst) - n_sub */
    int32_t window_mismatches;
} himut_support_row;
typedef struct himut_support_params {
    int32_t min_mapq, mismatch_window_size, reserved[2];
} himut_support_params;
int himut_run_support(himut_ctx* ctx, const int32_t* pos1, const uint8_t* ref, const uint8_t* alt, int64_t n_sites,
                      const himut_support_params* p);
int himut_get_support(himut_ctx* ctx, const himut_support_row** rows, int64_t* n_rows, const int32_t** site_counts);

/* ---- empirical base quality per reported BQ ("Row 8").  No counterpart inside the reference package:
 * its authors made the table with a script outside it (scripts/ccs2bq_calculation.py, get_bq2match_mismatch_count); what
 * is the reference's is the pile (caller.py:44-72) and the genotyper (gtlib.get_germ_gt, gtlib.py:122-135).
 * Inputs: himut_set_gt_lut, himut_set_chunks (the regions), himut_set_reference, the reads.  himut_set_params is not
 * needed and what it set is left alone.  The pile of a 0-based position p: every read that covers p (a read whose text
 * ends in an insertion also brings that insertion to its tend) with flag 0x100 clear and mapq >= min_mapq, in file order;
 * cells as update_allelecounts makes them (an insertion is counted at the position that follows it, a deletion at each
 * deleted position).  No other read filter; the pile never depends on the regions.  min_mapq = 0 is the script.
 * Positions swept: for every region (s, e) the 0-based positions s <= p < e (the script's range(chunk_start, chunk_end),
 * NOT the call run's 1-based inclusive rule); a position two regions hold is swept once per region.  Per position, in
 * this order: (1) the reference byte is not an upper-case A/C/G/T: skipped; (2) A+T+G+C+del >= md_threshold: skipped;
 * (3) ins != 0 or del != 0: skipped; (4) the column is genotyped (ordered fp64 sums in fetch order), gq < min_gq: skipped;
 * (5) if every A/T/G/C cell carries an allele of the genotype each of them adds one to match[its BQ], else the cells
 * whose allele is not in the genotype add one to mismatch[their BQ] and the genotype's own cells are counted nowhere
 * (the script's fall-through).  An empty column passes as homref by the prior and adds nothing.
 * Errors: HIMUT_ERR_ARG without tables, regions, reads or the reference string; HIMUT_ERR_CHUNK for a region with
 * start > end, start < 0 or end behind the reference string; HIMUT_ERR_BQ0 for a quality 0 in a column that reaches
 * step 4; HIMUT_ERR_BASE on the germline run's rule (a read with flag 0x100 clear, whatever its mapq, that overlaps a
 * region -- s < tend and e > tstart -- and holds an aligned base outside ATGC).
 * himut_get_bqcal: match[256] and mismatch[256] indexed by BQ (bin 0 stays 0); log[12]: positions swept, positions
 * skipped at steps 1, 2, 3, 4, positions that passed as homref, het, hetalt, homalt, positions that added only matches,
 * positions that added mismatches, 0.  Integer sums: two runs on the same input give the same numbers.
 * himut_get_records, himut_get_germline and himut_get_support keep serving their own last runs; the position bitmap,
 * the candidate mask and the scalars of the call and germline runs are left as found (the run has scalars of its own).
 * himut_get_stats after the run: ms_total, ms_parse and ms_eval (the sweep; stage timing 2), n_reads, read_bases,
 * positions = the positions swept. */
typedef struct himut_bqcal_params {
    int32_t min_mapq, min_gq, md_threshold, reserved[5];
} himut_bqcal_params;
int himut_run_bqcal(himut_ctx* ctx, const himut_bqcal_params* p);
int himut_get_bqcal(himut_ctx* ctx, int64_t match[256], int64_t mismatch[256], int64_t log[12]);
/* Test hook, no counterpart in the reference: how many pile rows of a tile the sweep of himut_run_bqcal holds in LDS at a
 * time (0: the default, all the kernel has room for).  A tile with more rows is staged in batches, and a second time
 * behind the verdict: a small value makes that path run on shallow piles.  Results never depend on it. */
int himut_debug_bqcal(himut_ctx* ctx, int row_batch);

/* ---- test hooks of the read pass (the cs decode in front of every pipeline), no counterpart in the reference.
 * himut_debug_decode: how the decode groups the reads.  0: the default, the tags of consecutive reads that fit 1 KB of
 * text are decoded by one wave.  1: every read on its own, through the per-read path.  Results never depend on it.  From
 * the call on the decode of this context counts its groups and keeps a copy of the position bitmap it set.
 * himut_debug_read_pass_sizes: out[3] = reads, slots of the segs / mis / mq arrays, words of the kept bitmap (0: the last
 * read pass was not a column front's).
 * himut_debug_read_pass: what the last read pass left, copied out.  Per read nseg, nmis, nnsub, rflag and meta (32 bytes:
 * int32 tstart, tend, nseg, uint32 flags, int64 segbase, qoff); the slot arrays whole -- a read's entries start at slot
 * (cs_off[r] >> 1) + r: nseg segments (int32 t0, q0, len, uint32 flags), nmis entries of mis and mq, and its nnsub
 * substitutions with an N reference base at mq[slot + (cs_off[r + 1] >> 1) - (cs_off[r] >> 1) - k]; slots no read uses hold
 * anything; bits (may be null): the bitmap; counters[4]: groups, groups of several reads, reads planned for the per-read
 * path (groups of one, groups that hold a secondary read), reads taken through it after the grouped path gave up on their
 * group; plan_ms: device time of the kernels that made the group plan of the batch. */
int himut_debug_decode(himut_ctx* ctx, int mode);
int himut_debug_read_pass_sizes(himut_ctx* ctx, int64_t out[3]);
int himut_debug_read_pass(himut_ctx* ctx, int32_t* nseg, int32_t* nmis, int32_t* nnsub, uint8_t* rflag, void* meta, void* segs,
                          int32_t* mis, uint32_t* mq, uint32_t* bits, int64_t counters[4], double* plan_ms);

/* ---- callable loci: the normcounts verdict of every swept position, as a map and as runs ("Row 9").
 * The reference has no counterpart: its worker (normcounts.py:206-421) folds the verdicts into two histograms and norm.log.
 * Inputs, read filters, pile, per-base callable bits, phase rule, order of tests and errors are himut_run_normcounts',
 * exactly: himut_set_params, himut_set_gt_lut, himut_set_chunks, himut_set_site_set, himut_set_phase (phased runs), the
 * reads, himut_set_reference; alt_order and non_human_sample as there.  HIMUT_ERR_ARG without any of them -- chunks
 * included: a run without chunks has no map -- and no kernel runs then.
 * For every chunk (s, e) and every 0-based position s <= rpos < e: a state, the row of norm.log the position adds its
 * bases to where there is one, and `bases`, the reference's tri_sum (the callable read bases over the position):
 *    0 NON_ACGT (reference byte not an upper-case A/C/G/T)   1 NO_BASE (tri_sum == 0)   2 UNPHASED   3 HET   4 HETALT
 *    5 HOMALT   7 INDEL   8 HIGH_DEPTH   9 ALLELE_BALANCE   10 LOW_GQ   11 PON   12 COMMON_SNP   13 CALLABLE
 * (6 is not used; bases is 0 for states 0 and 1).  The map holds the chunks' positions one behind the other in chunk
 * order: position rpos of chunk k is entry sum(e_j - s_j, j < k) + rpos - s_k; a position two chunks hold has two entries.
 * bases is a 16-bit field.  The sweep counts as the normcounts run does, in 32 bits at any depth; a position with more
 * than 65,535 callable bases cannot be stored and fails the run with HIMUT_ERR_DEPTH (nothing is saturated silently).
 * Runs: within one chunk the maximal stretches of equal state, ascending; runs never cross a chunk boundary (two chunks
 * that abut give two runs even where the state is the same) and come in chunk order.  bases: the int64 sum over the run.
 * log[14]: as himut_get_normcounts gives it for the same input.  Integer sums: two runs give the same bytes.
 * himut_get_callable: count-then-fetch as himut_get_support -- runs and n_runs are the library's, valid until the next
 * himut_run_callable or himut_destroy.  himut_get_callable_map copies the first n entries of the last run's map
 * (either pointer may be null); HIMUT_ERR_ARG before a run has completed or when n exceeds the positions it swept.
 * himut_get_records, himut_get_germline, himut_get_support, himut_get_bqcal and himut_get_normcounts keep serving their
 * own last runs.  himut_get_stats after the run: ms_total, ms_index (the read pass), ms_eval (the map sweep), ms_capture
 * (the run compaction), ms_finalize (the records' copy), positions = the positions swept, n_records = the runs. */
#define HIMUT_CALLMAP_TILE 256       /* positions a workgroup of the map sweep classifies at a time */
#define HIMUT_CALLMAP_BLOCK 2048     /* positions a workgroup of the run compaction scans */
enum {
    HIMUT_CM_NON_ACGT = 0, HIMUT_CM_NO_BASE = 1, HIMUT_CM_UNPHASED = 2, HIMUT_CM_HET = 3, HIMUT_CM_HETALT = 4,
    HIMUT_CM_HOMALT = 5, HIMUT_CM_INDEL = 7, HIMUT_CM_HIGH_DEPTH = 8, HIMUT_CM_ALLELE_BALANCE = 9, HIMUT_CM_LOW_GQ = 10,
    HIMUT_CM_PON = 11, HIMUT_CM_COMMON_SNP = 12, HIMUT_CM_CALLABLE = 13
};
typedef struct himut_callable_run {
    int32_t chunk;              /* index into the chunk list */
    int32_t start, end;         /* 0-based, half open */
    int32_t state;
    int64_t bases;
} himut_callable_run;
int himut_run_callable(himut_ctx* ctx, const uint8_t alt_order[12], int non_human_sample);
int himut_get_callable(himut_ctx* ctx, const himut_callable_run** runs, int64_t* n_runs, int64_t log[14]);
int himut_get_callable_map(himut_ctx* ctx, uint8_t* state, uint16_t* bases, int64_t n);

/* ---- the map per interval: callable counts and trinucleotide contexts of BED intervals ("Row 14").
 * Inputs: the map of the context's last completed himut_run_callable, with the chunk list and the reference length that
 * run saw (the callable run keeps a copy: a later himut_set_chunks changes nothing here), the context's reference string,
 * and n intervals (start[i], end[i]), 0-based and half open, in any order; they may overlap, nest, repeat, be empty
 * (start >= end) and reach outside every chunk or the contig.
 * HIMUT_ERR_ARG, before anything is queued: no callable run has completed or the last one failed; n < 0; an array is
 * null while n > 0; the reference string's length differs from the one the callable run saw.  n == 0 is a run with zero
 * rows.
 * A map entry of chunk k at position rpos belongs to interval i iff start[i] <= rpos < end[i]; a position two chunks hold
 * has two entries and counts twice, as in normcounts.  Intervals are independent of each other.  Row i, in input order:
 *    entries          the map entries in the interval
 *    positions[s]     those of state s (HIMUT_CM_*; index 6 stays 0)       bases[s]   the sum of their `bases`
 *    all_tri[33], ref_tri[33], ccs_tri[33]   histograms over the trinucleotide class of the entry's position: all_tri
 *                     counts every entry whatever its state; ref_tri adds 1 and ccs_tri adds `bases` for CALLABLE entries
 * The class: the key normcounts.get_tri_context gives -- the letters as the string holds them, case-sensitive; a key with
 * an upper-case purine centre is read on the other strand, any letter outside upper-case ACGT becoming N; NNN when
 * rpos - 1 < 0 or rpos + 2 > the string's length.  A key of the 32 with a C or T centre and ACGT on both sides has class
 * first * 8 + (centre == 'T' ? 4 : 0) + last with A0 C1 G2 T3; every other key has class 32.
 * All sums are integers: two runs give the same bytes.  The rows are the run's own: every other getter, himut_get_callable
 * and himut_get_callable_map included, keeps serving its last run.  himut_get_intervals: count-then-fetch as
 * himut_get_callable -- rows and n are the library's, valid until the next himut_run_intervals or himut_destroy.
 * himut_get_stats after the run: ms_total (device time: plan, scan, tally), n_records = n, positions = the map's entries. */
typedef struct himut_interval_row {
    int64_t entries;
    int64_t positions[14];
    int64_t bases[14];
    int64_t all_tri[33];
    int64_t ref_tri[33];
    int64_t ccs_tri[33];
} himut_interval_row;
int himut_run_intervals(himut_ctx* ctx, const int32_t* start, const int32_t* end, int64_t n);
int himut_get_intervals(himut_ctx* ctx, const himut_interval_row** rows, int64_t* n);

/* ---- somatic doublet base substitutions from the call path's pile ("Row 10").  `call` cannot report
 * one: a read with CC>TT proposes two single-base candidates inside each other's mismatch window (bamlib.py:266-282).  The
 * reference has a half-written tdbs_lst branch (cslib.cs2mut, cslib.py:67-150) that `call` never reaches.
 * Inputs: himut_set_params (all of call's thresholds; phase is ignored, as are phase sets), himut_set_gt_lut,
 * himut_set_chunks (the regions: they select which doublets are reported, they never shape a pile), himut_set_site_set
 * (either set may be empty or never set), the reads.  HIMUT_ERR_ARG without params, tables, regions or reads.
 * Pile of a 0-based position: every read with flag 0x100 clear that covers it, in file order, whatever its mapq; cells as
 * update_allelecounts makes them (caller.py:44-72).  Proposing reads: those that pass call's read filters
 * (caller.py:310-317); every alignment is a read of its own.  A doublet of a read, on cs2subindel's mismatch_lst
 * (cslib.py:47-64; letters upper-cased, substitutions with reference base N left out): two consecutive entries that are
 * substitutions at tpos and tpos + 1, the entry in front not a substitution at tpos - 1, the entry behind not one at
 * tpos + 2.  A run of three or more gives none and is counted once (num_mbs).  The read proposes (tpos, ref1 ref2, alt1
 * alt2) when neither qpos nor qpos + 1 is trimmed (bamlib.py:222-242) and, with (s1, e1) = get_mismatch_range(tpos, qpos,
 * qlen, w), (s2, e2) = get_mismatch_range(tpos + 1, qpos + 1, qlen, w), the entries of mismatch_lst with min(s1, s2) <=
 * position <= max(e1, e2), minus two, are <= max_mismatch_count.  Candidates: the distinct proposals with start <= tpos
 * <= end for some region, each evaluated once.
 * half_status[j]: the verdict call's non-phased cascade (caller.py:332-550) gives (tpos + j, ref_j, alt_j) on the pile,
 * with its germ_gq, genotype, state and six counts.  Joint counts over the pile reads (a read without an A/T/G/C cell at
 * a position has no allele there): both_alt, both_ref, one_alt (exactly one of the two alt alleles); n_proposers.
 * Verdict: a half dropped as germline (is_germ_gt): no record, counted (num_germ).  Else the half verdict that comes
 * first in HetSite, HetAltSite, HomAltSite, IndelSite, LowGQ, LowBQ, PanelOfNormal, ComSnp if a half holds one of them
 * (the first half on a tie); else LowDepth when both_ref < min_ref_count or both_alt < min_alt_count; else HighDepth when
 * a half is HighDepth; else PASS.  gq: the smaller half_gq.
 * Records: ascending by (tpos, alt1, alt2), alleles in ATGC order; two runs on the same input give the same bytes.
 * log[20]: proposing reads, runs of exactly two in them, num_mbs, doublets lost to trim, to the window (the five over all
 * proposing reads, whatever the regions); distinct candidates inside regions, num_germ; records by verdict in the order
 * HetSite, HetAltSite, HomAltSite, IndelSite, LowGQ, LowBQ, PanelOfNormal, ComSnp, LowDepth, HighDepth, PASS; 0, 0.
 * Errors: HIMUT_ERR_BQ0 for a quality 0 in a column of a candidate, HIMUT_ERR_BASE on the germline run's rule,
 * HIMUT_ERR_CS from the decode; the context stays usable.  himut_get_records, himut_get_germline and the other getters
 * keep serving their own last runs.  himut_get_stats after the run: ms_total, ms_capture, ms_parse / ms_index / ms_eval /
 * ms_finalize (stage timing 2), n_candidates = the proposals appended, n_records, column_slots, reran. */
typedef struct himut_dbs_record {
    int32_t tpos;               /* 1-based POS of the first base */
    int32_t gq;                 /* min(half_gq) */
    uint8_t ref[2], alt[2];     /* ASCII */
    uint8_t status;             /* HIMUT_ST_* */
    uint8_t half_status[2];
    uint8_t pad0;
    uint8_t gt_state[2];        /* 0 homref 1 het 2 hetalt 3 homalt */
    uint8_t gt[2][2];           /* per half the germline genotype, as himut_record's gt0, gt1 */
    uint8_t pad1[2];
    int32_t half_gq[2];
    uint32_t counts[2][6];      /* per half A T G C ins del, as himut_record's */
    uint32_t alt_bqsum[2];      /* per half the sum of BQ of its alt allele */
    uint32_t both_alt, both_ref, one_alt, n_proposers;
    uint32_t pad2[2];
} himut_dbs_record;             /* 112 bytes */
int himut_run_dbs(himut_ctx* ctx);
int himut_get_dbs(himut_ctx* ctx, const himut_dbs_record** records, int64_t* n, int64_t log[20]);

/* ---- the substitutions of a site list genotyped in this sample ("Row 11"): what the matched normal, or
 * another tissue of the donor, shows at each substitution `call` found elsewhere.  `call` only evaluates positions one of
 * this sample's reads proposes; the reference's authors looked sites up with pysam scripts outside the package.  What is
 * the reference's is the pile (caller.py:44-72), the genotyper (gtlib.get_germ_gt), is_germ_gt (caller.py:111-147) and the
 * non-phased cascade (caller.py:332-550).
 * Inputs: himut_set_params (min_gq, min_bq, min_mapq, min_ref_count, min_alt_count and md_threshold are read; phase is
 * ignored, as are phase sets), himut_set_gt_lut, himut_set_site_set (either set may be empty or never set), the reads, and
 * n_sites sites (pos1, ref, alt) under himut_run_support's rules: pos1 a 1-based VCF POS, non-decreasing; ref / alt ASCII
 * upper-case letters of ATGC, ref != alt; equal positions with other alleles and repeated triples are allowed, each site
 * is answered on its own; anything else is HIMUT_ERR_ARG.  HIMUT_ERR_ARG without params, tables or reads; n_sites == 0 is
 * a run with zero records.  himut_set_chunks is not needed and what it set is neither read nor changed: regions do not
 * exist for this run.
 * Pile of a site: every read with flag 0x100 clear that covers pos1 - 1 (tstart <= pos1 - 1 < tend; a read whose text ends
 * in an insertion also brings that insertion to its tend), in file order, whatever its mapq; cells as update_allelecounts
 * makes them (an insertion counts at the position that follows it, a deleted base is a del cell).  No read filter and no
 * chunk edge shape it.
 * One record per site, in input order (record[k] answers site k).  depth = A+T+G+C+del (bamlib.py:213-219).  depth == 0:
 * status HIMUT_ST_NOCOV, no genotype is taken, gq, gt_state and gt are 0 (the counts are still the column's: ins may be
 * set).  Else the genotype and gq of the shared genotype() (sums in fetch order, no contraction); is_germ_gt true: status
 * HIMUT_ST_GERMLINE (`call` drops such a candidate silently; here it is a record); else the first hit of HetSite,
 * HetAltSite, HomAltSite, IndelSite (ins or del != 0), LowGQ (gq < min_gq), LowBQ (no alt read with bq >= min_bq -- so a
 * site without any alt read is LowBQ unless an earlier rule holds), PanelOfNormal, ComSnp, LowDepth (ref count <
 * min_ref_count or alt count < min_alt_count), HighDepth (depth > md_threshold), PASS.
 * A site behind the span the position bitmap covers -- pos1 - 1 >= 256 * ((T >> 8) + 2), T the largest tend of the pushed
 * reads -- or on a batch without reads is a NoCoverage record with zero counts: no error, no out-of-range access.
 * log[20]: sites; NoCoverage; Germline; records by verdict in the order HetSite, HetAltSite, HomAltSite, IndelSite, LowGQ,
 * LowBQ, PanelOfNormal, ComSnp, LowDepth, HighDepth, PASS; sites with alt_count >= 1; distinct site positions inside the
 * span; 0, 0, 0, 0.  Integer sums: two runs on the same input give the same bytes.
 * Errors: HIMUT_ERR_BQ0 for a quality 0 in an A/T/G/C cell of a site's column; HIMUT_ERR_BASE for a query base outside ATGC
 * in a cell of a site's column (per column: a read with such a base elsewhere raises nothing); HIMUT_ERR_CS from the
 * decode.  The context stays usable after any of them.
 * himut_get_sites: records are the library's, valid until the next himut_run_sites or himut_destroy; the getters of all
 * other runs keep serving their own last runs.  himut_get_stats after the run: ms_total, ms_capture, ms_parse / ms_index /
 * ms_eval / ms_finalize (stage timing 2), n_reads, read_bases, n_candidates = n_records = n_sites, column_slots, reran. */
typedef struct himut_site_record {
    int32_t site;               /* index into the site arrays */
    int32_t tpos;               /* pos1 */
    uint8_t ref, alt;           /* ASCII, as given */
    uint8_t status;             /* HIMUT_ST_* */
    uint8_t gt_state;           /* 0 homref 1 het 2 hetalt 3 homalt */
    uint8_t gt[2];              /* the germline genotype, as himut_record's gt0, gt1; 0, 0 for NoCoverage */
    uint8_t pad[2];
    int32_t gq;
    uint32_t counts[6];         /* A T G C ins del, as himut_record's */
    uint32_t alt_bqsum, ref_bqsum;   /* sum of BQ of the alt allele's cells, of the reference allele's */
    uint32_t alt_hi;            /* alt reads with bq >= min_bq */
    uint32_t alt_mq;            /* alt reads with mapq >= min_mapq */
    uint32_t reserved;          /* 0 */
} himut_site_record;            /* 64 bytes */
int himut_run_sites(himut_ctx* ctx, const int32_t* pos1, const uint8_t* ref, const uint8_t* alt, int64_t n_sites);
int himut_get_sites(himut_ctx* ctx, const himut_site_record** records, int64_t* n, int64_t log[20]);

/* ---- germline short insertions and deletions ("Row 12").  The reference has no such run: in `call` an
 * indel only vetoes a site (IndelSite), and --germline_indel_prior is parsed and never read.  The contract is this text;
 * tests/indels_model.py states it in plain Python.
 * Inputs: the reads, himut_set_chunks (the regions: they select which alleles are evaluated, they never shape a pile),
 * himut_set_reference, and the parameter block below.  himut_set_params and himut_set_gt_lut are not needed and what they
 * set is neither read nor changed.  HIMUT_ERR_ARG without reads, regions or the reference string, and for max_len outside
 * 1..64; HIMUT_ERR_CHUNK for a region with start > end; no kernel is launched then.
 * The six doubles are the host's (math.log10, the GtLut precedent): with e the per-read indel error and pi the germline
 * indel prior, l_hit = log10(1 - e), l_err = log10(e), l_half = log10(0.5), prior = log10(1 - 1.5 pi), log10(pi),
 * log10(pi / 2) for homref, het, hom-alt.
 * Pile reads: flag 0x100 clear and mapq >= min_mapq; none of call's read filters.
 * Raw events of a pile read over [tstart, tend): every deletion of its cs text (p its first deleted 0-based position, L its
 * length, span end e_ = p + L) and every insertion (p the position it precedes, L its length, s its bases from SEQ, e_ =
 * p; insertions the text splits in a row are one).  In this order: an event without an aligned reference position of the
 * read on both sides (not tstart <= p - 1 and e_ < tend: a leading or trailing insertion, a deletion at an end) is no
 * event and is counted (num_edge); L > max_len is skipped and counted (num_long); an insertion that holds a base outside
 * ATGC is skipped and counted (num_nbase), no error.
 * Left-normalisation, against the reference string alone and whatever its case: while p - 1 > tstart and the byte at p - 1
 * is one of ACGT -- a deletion shifts if that byte equals the byte at p + L - 1, an insertion if it equals s[L - 1] -- p
 * goes down by one and an insertion's s is rotated right by one.  A byte behind the end of the string is no letter.  The
 * anchor is a = p - 1.  The shift stops at the read's own start, so every carrier spans its allele (n_alt <= DP) and a
 * read that begins inside a repeat can yield the same change under another anchor.
 * Alleles: (a, type, L, s), compared exactly.  Only alleles with start <= a <= end for some region are evaluated, each
 * once.  n_alt: the distinct reads with the allele (a read that yields it twice counts once and adds to num_dup).
 * n_other: the distinct reads with any event anchored at a, minus n_alt.  DP: the pile reads with tstart <= a and e_ <
 * tend (e_ = a + 1 + L for a deletion, a + 1 for an insertion).  n_non = DP - n_alt.
 * Genotype: states homref, het, hom-alt with per-read terms (x, y) = (l_hit, l_err), (l_half, l_half), (l_err, l_hit); in
 * fp64, in this order and without contraction: t = n_non * x; u = n_alt * y; sum = prior + t; sum = sum + u; PL = -10 *
 * sum.  The state is the smallest PL (ties: the lower index), gq the gap to the second smallest, truncated and capped at
 * 99 as the SNV genotyper's.  A homref allele gives no record unless report_homref (tests, bindings); its status is PASS
 * and no FILTER counter moves.  Else the first of LowGQ (gq < min_gq), LowDepth (n_alt < min_alt_count, or het and n_non
 * < min_ref_count), HighDepth (DP > md_threshold), PASS.
 * Records: ascending anchor, deletions before insertions, ascending L, the inserted string lexicographically in the code
 * order A T G C; two runs on the same input give the same bytes.  log[13]: events appended (normalised, inside a region),
 * alleles evaluated, num_edge, num_long, num_nbase (the three over all pile reads, whatever the regions), num_dup, homref,
 * het, hom-alt, PASS, LowGQ, LowDepth, HighDepth.
 * Errors: HIMUT_ERR_CS from the decode; the context stays usable.  The records are the library's, valid until the next
 * himut_run_indels or himut_destroy; the getters of all other runs keep serving their own last runs.  himut_get_stats after
 * the run: ms_total, ms_parse / ms_emit (the events) / ms_index (their sort and order) / ms_eval / ms_finalize (stage timing 2), n_reads,
 * read_bases, n_candidates = the events appended, n_records, reran (the events did not fit the capacity the previous
 * indels run left: the run was made again with exact sizes). */
typedef struct himut_indel_params {
    int32_t min_mapq;
    int32_t min_gq;
    int32_t min_ref_count;
    int32_t min_alt_count;
    int32_t md_threshold;
    int32_t max_len;            /* 1..64 */
    int32_t report_homref;      /* 0 / 1 */
    int32_t reserved;
    double l_hit, l_err, l_half;
    double prior[3];            /* homref het hom-alt */
} himut_indel_params;           /* 80 bytes */
typedef struct himut_indel_record {
    int32_t anchor;             /* a, 0-based: POS = anchor + 1 */
    int32_t len;                /* L */
    uint8_t type;               /* 0 deletion, 1 insertion */
    uint8_t status;             /* HIMUT_ST_* */
    uint8_t gt_state;           /* 0 homref 1 het 2 hom-alt */
    uint8_t pad0;
    int32_t gq;
    uint32_t dp, n_alt, n_other;
    uint32_t pad1;
    uint8_t bases[16];          /* the inserted bases as 2-bit codes A0 T1 G2 C3, base i at bits 2 (i & 3) of byte i >> 2; 0 for a deletion */
    uint32_t reserved[4];       /* 0 */
} himut_indel_record;           /* 64 bytes */
int himut_run_indels(himut_ctx* ctx, const himut_indel_params* p);
int himut_get_indels(himut_ctx* ctx, const himut_indel_record** records, int64_t* n, int64_t log[13]);

/* ---- empirical indel error per homopolymer run of the reference ("Row 13").  The reference has no such
 * run.  It measures, on this BAM, what himut_run_indels takes as one constant (l_hit, l_err): per class of run, how many
 * pile reads span a run and how many indel events they show in it.  Integers only; the contract is this text, and
 * tests/indelcal_model.py states it in plain Python.
 * Inputs: those of himut_run_indels -- the reads, himut_set_chunks, himut_set_reference -- and the block below.
 * HIMUT_ERR_ARG without reads, regions or the reference string, for max_len outside 1..64, min_alt_count < 0 and
 * vaf_permille outside 0..1000; HIMUT_ERR_CHUNK for a region with start > end; no kernel is launched then.
 * Pile reads, raw events, their three rules (num_edge, num_long, num_nbase), left-normalisation, the anchor a and the
 * region test are himut_run_indels' under the same min_mapq and max_len; so are an allele's n_alt and DP.
 * Runs: reference bytes are compared upper-cased.  A run is a maximal stretch [s, s + n) of one letter b of ACGT with
 * s >= 1 and s + n < reflen: a position on either side, whatever its byte.  Its anchor is a = s - 1.  A run is considered
 * if start <= a <= end for some region, once however the regions overlap.  A considered run with n > 64 is counted in
 * runs_long and takes no further part.  The class of any other: c = code(b) * 32 + min(n, 32) - 1 with A T G C = 0..3:
 * 128 classes, the last length bin holds 32..64.
 * Variant anchors: anchor a is variant if some allele there has n_alt >= min_alt_count and n_alt * 1000 >= vaf_permille *
 * DP.  A considered run whose anchor is variant is excluded: it counts in runs[c] and excluded[c] and adds neither spans nor
 * events.  The threshold is a definition; in very long runs true error can exceed it, which biases those rows low, and
 * runs and excluded side by side show how much of a class was set aside.
 * Spans: a considered run that is neither long nor excluded adds to spans[c] the pile reads with tstart <= s - 1 and
 * s + n < tend, whatever the reads' lengths.
 * Events: every event the front collects (normalised, anchor inside a region), in this order: if a is variant it counts in
 * events_variant.  Else, with b the upper-cased byte at a + 1: num_offrun if b is not of ACGT, if the upper-cased byte at
 * a equals b (the shift stopped at the read's start, at position 1 or at an N), or if the run at a + 1 is longer than 64 or
 * has no position behind it.  Else, n being that run's length: num_partial unless a + 1 + n < tend of the event's read.
 * Else it counts in class c under one of seven columns: del1, del2, del3p -- a deletion with L <= n, by min(L, 3); ins1,
 * ins2, ins3p -- an insertion whose bases all equal b, by min(L, 3); other -- a deletion with L > n or an insertion with
 * another base.  Events are counted, not reads: "+ac-gt" at one anchor is two events against one span.
 * himut_get_indelcal: table[c * 10 + k], k = runs, excluded, spans, del1, del2, del3p, ins1, ins2, ins3p, other; log[14]:
 * events, num_edge, num_long, num_nbase (as himut_run_indels counts them), anchors (distinct anchors of the events),
 * variant_anchors, events_variant, num_offrun, num_partial, events_counted, runs, runs_excluded, runs_long, spans.
 * events = events_variant + num_offrun + num_partial + events_counted; the seven event columns sum to events_counted, the
 * runs, excluded and spans columns to runs, runs_excluded and spans.  Nothing ran yet: zeros.
 * The run keeps an event list, a bitmap and scalars of its own: every other getter keeps serving its last run.
 * Errors, kept capacities and himut_get_stats are himut_run_indels' (reran: the events did not fit what the previous
 * indelcal run left); of the stage times ms_hap is the variant marks, ms_eval the event pass, ms_finalize the span sweep,
 * n_candidates the events, n_records 0.
 *
 * himut_set_indel_error_table: the per-read terms himut_run_indels uses in place of its constants l_hit and l_err, one pair
 * per cell c * 7 + k of (class, event column): an allele (a, type, L, s) is classified as an event is -- the run at a + 1
 * and the column, without the event's read -- and an allele with no class (off run) keeps the constants.  The fp64
 * operations and their order do not change.  The doubles are the host's (math.log10 of 1 - e and of e); n is
 * HIMUT_INDEL_ERROR_CELLS, or 0 to clear (l_hit and l_err are not read then); anything else is HIMUT_ERR_ARG.  The table
 * stays until it is cleared; himut_run_indels and himut_run_sindels read it. */
#define HIMUT_INDELCAL_CLASSES 128
#define HIMUT_INDELCAL_COLS 10
#define HIMUT_INDEL_ERROR_CELLS 896
typedef struct himut_indelcal_params {
    int32_t min_mapq;
    int32_t max_len;            /* 1..64 */
    int32_t min_alt_count;
    int32_t vaf_permille;       /* 0..1000 */
    int32_t reserved[4];
} himut_indelcal_params;        /* 32 bytes */
int himut_run_indelcal(himut_ctx* ctx, const himut_indelcal_params* p);
int himut_get_indelcal(himut_ctx* ctx, int64_t table[1280], int64_t log[14]);
int himut_set_indel_error_table(himut_ctx* ctx, const double* l_hit, const double* l_err, int64_t n);
/* Test hook, no counterpart in the reference: the workgroups of the span sweep of himut_run_indelcal (0 = eight per CU;
 * fewer than the region's 256-position blocks make a workgroup sweep several) and what a 32-bit cell of a workgroup's
 * histogram may hold before it is added to the table (0 = 2^31).  The results do not depend on either. */
int himut_debug_indelcal(himut_ctx* ctx, int sweep_workgroups, int64_t cell_budget);

/* ---- somatic indel candidates carried by single reads ("Row 16").  The reference has no such run.  HiFi
 * indel error outside repeats is orders of magnitude above a somatic indel rate and higher still inside homopolymers, so
 * the records are candidates under the rules below, not calls; the counters are what a user needs to subtract an expected
 * error load (himut_run_indelcal gives the rate).  The contract is this text; tests/sindels_model.py states it in plain
 * Python.
 * Inputs: those of himut_run_indels -- the reads, himut_set_chunks, himut_set_reference, optionally the table of
 * himut_set_indel_error_table -- and the block below.  himut_set_params, the genotype table and the site sets are neither
 * read nor changed.
 * Pile reads, raw events, their three rules (num_edge, num_long, num_nbase), the left-normalisation, the region test,
 * alleles, n_alt, n_other and DP are himut_run_indels' under the same min_mapq and max_len.
 * Proposing reads: the pile reads that pass call's read filters (caller.py:310-317): the identity of the cs text is not
 * below min_sequence_identity; sum(bq) >= min_qv * qlen in integers, over the whole query, soft clips included; mapq >=
 * min_mapq; qlen_lower_limit < qlen < qlen_upper_limit.
 * Per-event rules, on an event of a proposing read that passed the three rules above, whatever the regions, on the raw
 * (unshifted) event: p its first deleted position or the position the insertion precedes, q the query offset its entry
 * of cs2subindel's mismatch list carries (an insertion's first base, the query base behind a deletion), L its length.
 * The footprint is the query interval [qa, qb], qa = q - 1, qb = q for a deletion and q + L for an insertion: the aligned
 * bases on either side and the inserted ones.  The first of these that fails is counted: num_trim -- qa or qb is trimmed
 * (bamlib.py:222-242: x < floor(min_trim qlen) or x > ceil((1 - min_trim) qlen), in doubles); num_window -- with (s, e) =
 * get_mismatch_range(p + 1, q, qlen, mismatch_window_size) (bamlib.py:245-258) the entries of the read's mismatch list
 * with s <= position <= e, minus one, exceed max_mismatch_count ("+ac-gt" is two entries at one place: each vetoes the
 * other at 0); num_lowbq -- a base of the footprint has bq < min_bq.  An event that passes proposes its left-normalised
 * allele.
 * Candidates: the distinct alleles with at least one proposing event and start <= a <= end for some region; each is
 * evaluated once.  n_prop: the distinct reads with a proposing event of the allele.
 * Genotype: himut_run_indels' three states and gq, on n_non = DP - n_alt and n_alt; under a table the allele's cell gives
 * l_hit and l_err as there.
 * Verdict, the first hit: the state is not homref -- dropped as germline, no record, counted (num_germ_het,
 * num_germ_homalt); IndelSite (HIMUT_ST_INDEL) -- n_other > 0; Repeat (HIMUT_ST_REPEAT) -- the homopolymer run of the
 * reference that starts at a + 1 is longer than 64, or the allele has a class (row 13: a run of 1..64 with a position
 * behind it) whose column is not "other" (a deletion inside the run, an insertion of the run's letter alone) and the run
 * is longer than max_run; repeats of longer units are not recognised; LowGQ -- gq < min_gq; LowDepth -- n_alt <
 * min_alt_count or DP - n_alt - n_other < min_ref_count; HighDepth -- DP > md_threshold; PASS.
 * Records: himut_run_indels' order; two runs on the same input give the same bytes.  log[20]: events (normalised, inside a
 * region, of all pile reads), num_edge, num_long, num_nbase, pile reads, proposing reads, events of proposing reads (past
 * the three rules, whatever the regions), num_trim, num_window, num_lowbq, proposing events, candidates, num_germ_het,
 * num_germ_homalt, IndelSite, Repeat, LowGQ, LowDepth, HighDepth, PASS.  log[6] = log[7] + log[8] + log[9] + log[10];
 * log[11] = log[12] + ... + log[19] = log[12] + log[13] + the records.
 * Errors: HIMUT_ERR_ARG without reads, regions or the reference string, for max_len outside 1..64, min_trim outside
 * [0, 0.5], and a negative max_run, mismatch_window_size or max_mismatch_count; HIMUT_ERR_CHUNK for a region with start >
 * end; no kernel is launched then.  HIMUT_ERR_CS from the decode.  The context stays usable.  The records are the
 * library's, valid until the next himut_run_sindels or himut_destroy; the getters of all other runs keep serving their
 * own last runs.  himut_get_stats: as himut_run_indels, with ms_hap the reads' verdicts (k_sindel_reads: every quality
 * once); reran: the events did not fit what the previous sindels run left. */
typedef struct himut_sindel_params {
    int32_t min_mapq;
    int32_t min_gq;
    int32_t min_ref_count;
    int32_t min_alt_count;
    int32_t md_threshold;
    int32_t max_len;            /* 1..64 */
    int32_t max_run;            /* >= 0 */
    int32_t min_qv;
    double l_hit, l_err, l_half;
    double prior[3];            /* homref het hom-alt */
    int32_t qlen_lower_limit, qlen_upper_limit;
    int32_t min_bq;
    int32_t mismatch_window_size;
    int32_t max_mismatch_count;
    int32_t reserved;
    double min_sequence_identity;
    double min_trim;            /* 0..0.5 */
} himut_sindel_params;          /* 120 bytes */
typedef struct himut_sindel_record {
    int32_t anchor;             /* the fields of himut_indel_record at its offsets; gt_state is 0 */
    int32_t len;
    uint8_t type;
    uint8_t status;             /* HIMUT_ST_* */
    uint8_t gt_state;
    uint8_t pad0;
    int32_t gq;
    uint32_t dp, n_alt, n_other;
    uint32_t pad1;
    uint8_t bases[16];
    uint32_t n_prop;            /* distinct reads with a proposing event of the allele */
    uint8_t run_base;           /* the run that starts at a + 1: its letter A0 T1 G2 C3 and min(length, 65); 0, 0 where none starts */
    uint8_t run_len;
    uint8_t class_col;          /* del1 del2 del3p ins1 ins2 ins3p other as 0..6 where the allele has a class, else 255 */
    uint8_t pad2;
    uint32_t reserved[2];       /* 0 */
} himut_sindel_record;          /* 64 bytes */
int himut_run_sindels(himut_ctx* ctx, const himut_sindel_params* p);
int himut_get_sindels(himut_ctx* ctx, const himut_sindel_record** records, int64_t* n, int64_t log[20]);

/* ---- each read's haplotype from the contig's phased hetSNPs ("Row 15").  No counterpart inside the
 * reference package: its authors assigned molecules with a script outside it (scripts/sbs2hap.py); haplib.get_ccs_hap
 * (k_read_hap) answers per (chunk, read) with one all-or-nothing byte that never leaves the device.
 * Inputs: the reads, n hetSNPs as parallel arrays, a parameter struct.
 *    pos1      1-based, strictly ascending
 *    ref, alt  ASCII, one of upper-case ACGT each, ref != alt
 *    bit       0 for GT 0|1, 1 for 1|0: the allele on the first haplotype
 *    set       the hetSNP's phase set, 0 <= set < n_sets; sets may interleave in position order
 *    params    min_snps >= 1, min_agree_permille in 501..1000
 * A null pointer (an array while n > 0, params), n < 0, n_sets < 0, an array that breaks one of these rules or a
 * parameter out of range is HIMUT_ERR_ARG with a message that names the rule; no kernel runs and the context stays
 * usable.  n == 0 is a valid run, and so is a context whose pushed or ingested batch holds no reads (zero rows); a context
 * nothing was ever pushed to is HIMUT_ERR_ARG, as for every other run.  himut_set_params, the genotype table, chunks, site
 * sets, himut_set_phase and the reference string are neither needed nor read.
 * Pile reads: flag 0x100 clear and mapq >= min_mapq (the germline and indels runs' rule).  A pile read spans hetSNP k iff
 * tstart <= pos1[k] - 1 < tend.  At a spanned hetSNP the first rule that matches classifies the read:
 *    1. the position lies in a deletion: del       2. the base's quality is < min_bq: lowbq
 *    3. the query base is ref: allele 0; alt: allele 1 -- a vote for haplotype allele XOR bit[k]
 *    4. anything else (an N in SEQ included): other
 * A spanned position no segment of the read holds (no well-formed cs text has one) fails the run with HIMUT_ERR_COVER.
 * One himut_haplotag_row per pushed read, in read order (row i: read i), non-pile reads included:
 *    set       the chosen phase set: of the sets with a vote of this read the one with the most votes, the lower index on
 *              a tie; -1 without a vote
 *    n0, n1    the read's votes for haplotype 0 and 1 among the hetSNPs of the chosen set
 *    n_other, n_del, n_lowbq   over the chosen set's spanned hetSNPs; with set == -1 over all spanned hetSNPs
 *    n_sets    the distinct sets with at least one vote of the read, capped at 65,535
 *    hap       0, 1, or 2 for none
 *    status    the first that applies: HIMUT_HT_NOTINPILE (every count 0), NOSNP (spans no hetSNP), NOVOTE (spans some, none
 *              voted), LOWSUPPORT (n0 + n1 < min_snps), CONFLICT (n0 == n1, or max(n0, n1) * 1000 <
 *              min_agree_permille * (n0 + n1) as 64-bit integers), ASSIGNED (hap: the larger count)
 * One himut_haplotag_snp per hetSNP: n_ref, n_alt, n_other, n_del, n_lowbq over the pile reads that span it (their sum is
 * its spanning depth); agree / disagree over the ASSIGNED reads whose chosen set is the hetSNP's set and that voted at it:
 * the vote equals the read's hap, or not.  agree + disagree <= n_ref + n_alt.
 * log[13]: reads, pile, hap0, hap1, NoSnp, NoVote, LowSupport, Conflict, multi_set (reads with n_sets >= 2), then votes,
 * other, del, lowbq summed over all (pile read, spanned hetSNP) pairs, whatever the chosen sets.
 * Everything is an integer: two runs give the same bytes.  himut_get_haplotag: rows, snps and log are the library's host
 * copies, valid until the next himut_run_haplotag or himut_destroy (any out pointer may be null); a run that failed
 * leaves the previous run's.  The run keeps buffers and scalars of its own: every other getter keeps serving its last run.
 * A substitution whose cs text names a base outside ACGT fails in the decode, as in every run (HIMUT_ERR_BASE).
 * himut_get_stats after the run: ms_total, from stage timing 2 ms_parse (the clearing and the decode) and ms_eval (the rows,
 * the tallies, the counters); n_reads, read_bases, n_records = rows, positions = n. */
enum {
    HIMUT_HT_ASSIGNED = 0, HIMUT_HT_NOTINPILE = 1, HIMUT_HT_NOSNP = 2, HIMUT_HT_NOVOTE = 3, HIMUT_HT_LOWSUPPORT = 4,
    HIMUT_HT_CONFLICT = 5
};
/* himut_haplotag_row, 32 bytes: read @0, set @4, n0 @8, n1 @12, n_other @16, n_del @20, n_lowbq @24, n_sets @28 (16 bit),
 * hap @30, status @31 */
typedef struct himut_haplotag_row {
    int32_t read;
    int32_t set;
    uint32_t n0;
    uint32_t n1;
    uint32_t n_other;
    uint32_t n_del;
    uint32_t n_lowbq;
    uint16_t n_sets;
    uint8_t hap;
    uint8_t status;
} himut_haplotag_row;
/* himut_haplotag_snp, 32 bytes: eight 32-bit words */
typedef struct himut_haplotag_snp {
    uint32_t n_ref;
    uint32_t n_alt;
    uint32_t n_other;
    uint32_t n_del;
    uint32_t n_lowbq;
    uint32_t agree;
    uint32_t disagree;
    uint32_t pad;               /* zero */
} himut_haplotag_snp;
typedef struct himut_haplotag_params {
    int32_t min_mapq;
    int32_t min_bq;
    int32_t min_snps;           /* >= 1 */
    int32_t min_agree_permille; /* 501..1000 */
    int32_t reserved[4];
} himut_haplotag_params;        /* 32 bytes */
int himut_run_haplotag(himut_ctx* ctx, const int32_t* pos1, const uint8_t* ref, const uint8_t* alt, const uint8_t* bit,
                       const int32_t* set, int64_t n, int32_t n_sets, const himut_haplotag_params* p);
int himut_get_haplotag(himut_ctx* ctx, const himut_haplotag_row** rows, int64_t* n_rows, const himut_haplotag_snp** snps,
                       int64_t* n_snps, int64_t log[13]);
/* ---- substitutions on both strands of one molecule ("Row 19").  `ccs --by-strand` writes two reads per
 * molecule, one per DNA strand; a mutation sits on both, polymerase error and base damage on one.  No counterpart in the
 * reference package, which takes every alignment as a molecule of its own.
 * Inputs: himut_set_params (every field but phase and min_hap_count is read), himut_set_gt_lut, himut_set_chunks, the site
 * sets (either may be empty or never set), the reads, mate[n_reads] and a parameter block of reserved words (all zero).
 * HIMUT_ERR_ARG without params, tables, reads or chunks.
 *    mate[i]   the read on the other strand of read i's molecule, or -1.  Checked on the host before any kernel is queued:
 *              an entry outside -1..n-1, mate[i] == i, or mate[mate[i]] != i is HIMUT_ERR_ARG with a message that names
 *              the read, as are n_mate != n_reads, a null mate while n_reads > 0 and a reserved word that is not zero.  The
 *              context stays usable.  A pair is counted once (log: pairs).
 * Positions: p is 0-based (p + 1 is the VCF POS, a record's tpos); "inside a chunk": start <= p < end for some chunk.
 * Pile reads: flag 0x100 clear and mapq >= min_mapq.  A read proposes when it is a pile read and passes call's read
 * filters (caller.py:310-317, himut_run_sindels' wording): identity >= min_sequence_identity, sum of its qualities >=
 * min_qv * qlen, qlen_lower_limit < qlen < qlen_upper_limit.  A pair is in play when both reads propose; any other pair
 * is counted under the first cause, in this order, that either read shows: not a pile read, identity, quality sum, query
 * length.
 * Events of a read A of a pair in play: every substitution of its mismatch list (cs2subindel's, cslib.py:47-64: letters
 * upper-cased, a substitution whose reference base is N left out), as (p, ref, alt, qa), qa the query offset.  A's own
 * rules, the first that fails counted: num_trim (qa < floor(min_trim * qlen) or qa > ceil((1 - min_trim) * qlen),
 * bamlib.py:222-242), num_window (the entries of A's mismatch list in get_mismatch_range(p + 1, qa, qlen,
 * mismatch_window_size), minus the event's own, exceed max_mismatch_count: himut_run_support's window_mismatches),
 * num_lowbq (bq[qa] < min_bq).
 * An event that passes meets the mate B at p; B's state is the first that matches:
 *    nocover     not (B.tstart <= p < B.tend)          del     p lies in a deletion of B
 *    lowbq       B's quality at its offset qb < min_bq   trim    qb is trimmed (B's qlen)
 *    concordant  B's query base is alt                   single  it is ref        other  anything else
 * (a spanned position no segment of B holds fails the run with HIMUT_ERR_COVER, as in himut_run_haplotag).
 * A concordant event is a double-strand event when B's own entry at p passes B's window rule too (its trim and quality
 * rules are the states above); else num_mate_window.  Both reads see a double-strand event; it is counted once, from the
 * read with the lower index.
 * Candidates: the distinct (p, ref, alt) with at least one double-strand event inside a chunk, each evaluated once.  The
 * first 64 bytes of a record are, field for field, the himut_site_record that himut_run_sites returns for (p + 1, ref, alt)
 * on the same reads, params and site sets (site: the record's index): the same kernels over the same column front.  That
 * pile holds EVERY read with flag 0x100 clear: both reads of a molecule are in it, a molecule in play counts twice in
 * counts[], and an alt_count of 2 can be one molecule.  Behind them:
 *    n_ds            molecules (pairs in play) with a double-strand event of the allele
 *    n_ss            events (p, ref, alt) of reads in play that pass their own rules and meet a `single` mate
 *    n_alt_unpaired  pile reads whose mismatch list holds (p, ref, alt) and that are in no pair in play (no rule applied)
 * Records ascend by (tpos, ref, alt), alleles in the order A T G C.
 * ss[12]: the `single` events inside a chunk by the change on the read's own strand -- a read with flag 0x10 adds
 * complement(ref) > complement(alt) -- in the order A>C A>G A>T C>A C>G C>T G>A G>C G>T T>A T>C T>G.  No site set applies.
 * ds_bases: the (pair in play, p inside a chunk) at which both reads hold an aligned base (a match or a substitution, not
 * a deletion), both qualities are >= min_bq and neither offset is trimmed.  The mismatch window is NOT applied, so the
 * count is an upper bound of the positions at which a double-strand event could have been seen.  ds_pairs_overlap: the
 * pairs with at least one such position.
 * log[40]:  0 reads  1 pile_reads  2 proposing_reads  3 pairs  4 pairs_in_play  5 pairs_notpile  6 pairs_identity
 *    7 pairs_lowqv  8 pairs_qlen  9 events (of reads in play)  10 num_trim  11 num_window  12 num_lowbq  13 nocover  14 del
 *    15 lowbq  16 trim  17 concordant  18 single  19 other  20 num_mate_window  21 ds_events  22 ds_events_in_chunk
 *    23 ss_events_in_chunk  24 ds_bases  25 ds_pairs_overlap  26 candidates  27 Germline  28..38 the verdicts in the order
 *    HetSite HetAltSite HomAltSite IndelSite LowGQ LowBQ PanelOfNormal ComSnp LowDepth HighDepth PASS  39 reserved (0).
 * Identities:  [3] = [4] + [5] + [6] + [7] + [8];  [9] = [10] + [11] + [12] + [13] + ... + [19];
 *    [17] = 2 * [21] + [20];  [26] = [27] + ... + [38] = records;  [23] = the sum of ss[];  [22] = the sum of n_ds.
 * Everything is an integer: two runs give the same bytes.  Errors of the decode and of the columns as in himut_run_sites.
 * himut_get_duplex: records are the library's, valid until the next himut_run_duplex or himut_destroy; ss and log may be
 * null; the getters of all other runs keep serving their own last runs.  himut_get_stats after the run: ms_total,
 * ms_capture, from stage timing 2 ms_parse, ms_hap (the pair kernels, the host's waits for their counts included),
 * ms_index, ms_eval, ms_finalize; n_reads, read_bases, positions, n_candidates = n_records, column_slots, reran (a key or
 * column buffer kept from the previous run had to grow). */
typedef struct himut_duplex_params {
    int32_t reserved[8];        /* 0 */
} himut_duplex_params;          /* 32 bytes */
typedef struct himut_duplex_record {
    himut_site_record site;     /* the sites run's record of (tpos, ref, alt) */
    uint32_t n_ds;
    uint32_t n_ss;
    uint32_t n_alt_unpaired;
    uint32_t reserved;          /* 0 */
} himut_duplex_record;          /* 80 bytes */
int himut_run_duplex(himut_ctx* ctx, const int32_t* mate, int64_t n_mate, const himut_duplex_params* p);
int himut_get_duplex(himut_ctx* ctx, const himut_duplex_record** records, int64_t* n, int64_t ss[12], int64_t log[40]);

/* tstart, tend, the SAM flag and mapq of the context's reads, pushed or ingested, in read order (n_reads each; a null
 * pointer leaves that array out): what a table with a line per read says beside a run's row (`himut haplotag`); the
 * ingest keeps them on the device.  HIMUT_ERR_ARG on a context nothing was pushed to. */
int himut_get_read_info(himut_ctx* ctx, int32_t* tstart, int32_t* tend, uint16_t* flag, uint8_t* mapq);

/* Dense pile of [p0, p1) over ALL pushed reads (no chunk restriction):
 * counts[(p - p0) * 6 + a], bqsum[(p - p0) * 4 + b]  (caller.py:44-72). */
int himut_pile_counts(himut_ctx* ctx, int32_t p0, int32_t p1, uint32_t* counts, uint32_t* bqsum);

#ifdef __cplusplus
}
#endif
#endif
