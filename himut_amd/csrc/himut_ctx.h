// Host side of libhimut_hip.so, the C ABI of include/himut_hip.h: what its source files share.  One file per pipeline,
// each launching the kernels of its own device header on the context's stream:
//
//   himut_ctx.hip     the context, the setters, the read batch, the chunk tables, the pinned staging windows
//   himut_front.hip   the read pass every pipeline starts with (himut_reads.h); the column front the call, germline, dbs
//                     and sites runs share, tail and stage times included (front_*, himut_front.h)
//   himut_call.hip    the call run (himut_call.h): do_run_once = call_plan (the sizes, every buffer;
//                     call_reserve_records lists the ones the candidate count sizes), the front, call_candidates,
//                     call_eval, call_finalize, the front's tail, and finish_run for the host's half; its records and
//                     counters
//   himut_pile.hip    the dense pile of himut_pile_counts (himut_pile.h)
//   himut_norm.hip    normcounts (himut_norm.h, himut_normq.h): a loop of passes (do_normcounts), each norm_plan (the
//                     sizes, every buffer), norm_read_pass, norm_sweep_quad or norm_sweep_tile, norm_finish.  The
//                     kernels' arguments, the classification of a position and the tile sweep, which the callable
//                     run's map sweep inlines too: himut_sweep.h
//   himut_ingest.hip  the device-side BAM ingest (himut_ingest.h)
//   himut_mut.hip     trinucleotide and SBS counts, phase edges (himut_fasta.h, himut_edges.h)
//   himut_spectra.hip the ID83 classes of a list of indel alleles over the resident string, the DBS78 classes of a list
//                     of doublets (himut_spectra.h)
//   himut_fit.hip     signature exposures of a spectrum and of its bootstrap replicates (himut_fit.h)
//   himut_germ.hip    the germline run (himut_germ.h)
//   himut_support.hip the reads that carry the substitutions of a site list (himut_support.h)
//   himut_bqcal.hip   the bqcal run: matches and mismatches per reported base quality (himut_bqcal.h)
//   himut_callmap.hip the callable run: a state per swept position and its runs (himut_callmap.h, over himut_sweep.h),
//                     behind normcounts' front
//   himut_intervals.hip the intervals run: the callable run's map tallied per interval (himut_intervals.h)
//   himut_dbs.hip     the dbs run: doublet base substitutions (himut_dbs.h), behind the column front
//   himut_sites.hip   the sites run: a site list genotyped on the pile (himut_sites.h), over the column front with the
//                     bitmap filled from the sites
//   himut_indels.hip  the indels run: short insertions and deletions from the decoded reads (himut_indels.h), behind
//                     the cs decode alone; the ordered events both it and the indelcal run start from (indel_front_run)
//   himut_indelcal.hip the indelcal run: indel events and spanning reads per homopolymer run of the reference
//                     (himut_indelcal.h), behind the indels run's ordered events; the table the indels run may read
//   himut_sindels.hip the sindels run: somatic indel candidates carried by single reads (himut_sindels.h), behind the
//                     indels run's ordered events with the reads' verdicts and the per-event rules added
//   himut_haplotag.hip the haplotag run: each read's haplotype from the phased hetSNPs, the reads' tallies per hetSNP
//                     (himut_haplotag.h), behind the cs decode alone
//   himut_duplex.hip  the duplex run: substitutions that both reads of a molecule show (himut_duplex.h), its candidates
//                     genotyped by the sites run's pass
// The call, germline, dbs and sites kernels that genotype a column of the column store inline one column walk, one
// genotype and one verdict cascade: himut_column.h; where their records go and how they are moved to the front in order:
// himut_emit.h.  The dense pile (k_pile_dense) and the bqcal sweep (k_bqcal) stage their pile rows into LDS through one
// pile tile: himut_piletile.h.  The runs' checks of what the context holds (check_run_inputs), the site list of the support
// and sites runs (encode_sites) and a run's result block on the host (RunOut: begin_run, take_log, get_run_out): below.
//
// The code the compiler makes of a kernel can depend on what shares its unit: a kernel that moves to another file is
// checked by comparing the compiler's output of the two builds (profiles/README.md).
// No torch types, no C++ exceptions across the boundary (guarded).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "himut_hip.h"
#include "himut_device.h"

namespace himut {

struct HipFail {
    hipError_t e;
    const char* what;
    const char* file;
    int line;
};

#define HCHECK(expr)                                   \
    do {                                               \
        hipError_t _e = (expr);                        \
        if (_e != hipSuccess) throw himut::HipFail{_e, #expr, __FILE_NAME__, __LINE__}; \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    uint64_t gen = 0;      // counts the allocations: a block that was freed and allocated again may come back at the SAME address,
                           // with other contents -- who keeps track of what a buffer holds compares this, not the pointer
    ~DevBuf() { if (p) (void)hipFree(p); }
    void reserve(size_t bytes) {
        if (bytes <= cap && p) return;
        // growing = free + allocate.  Work already queued on the context's (non-blocking) streams may still use the
        // old block, so the device is drained first; this happens when a contig is larger than the ones before it.
        if (p) { HCHECK(hipDeviceSynchronize()); HCHECK(hipFree(p)); p = nullptr; cap = 0; }
        size_t want = std::max<size_t>(bytes, 256);
        HCHECK(hipMalloc(&p, want));
        cap = want; gen++;
    }
    // grows to at least `bytes` keeping the first `used` bytes (the ingest's arrays grow while they are being filled)
    void grow_keep(size_t bytes, size_t used) {
        if (bytes <= cap && p) return;
        const size_t want = std::max<size_t>(std::max(bytes, cap + cap / 2), 256);
        void* q = nullptr;
        HCHECK(hipDeviceSynchronize());
        HCHECK(hipMalloc(&q, want));
        if (p && used) HCHECK(hipMemcpy(q, p, std::min(used, cap), hipMemcpyDeviceToDevice));
        if (p) HCHECK(hipFree(p));
        p = q; cap = want; gen++;
    }
    void release() {
        if (p) { HCHECK(hipDeviceSynchronize()); HCHECK(hipFree(p)); p = nullptr; cap = 0; }
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

template <class T>
void upload(DevBuf& b, const T* src, size_t n, hipStream_t st) {
    b.reserve(std::max<size_t>(n, 1) * sizeof(T) + 256);  // slack: kernels read whole 16/32-byte windows
    if (n) HCHECK(hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, st));
}

template <class T>
void upload(DevBuf& b, const std::vector<T>& v, hipStream_t st) { upload(b, v.data(), v.size(), st); }

enum { EV_START = 0, EV_SIDE, EV_PARSE, EV_HAP, EV_EMIT, EV_INDEX, EV_GATHER, EV_SWEEP, EV_FINAL, EV_COPIED, EV_COUNT };

// scalars block in device memory
struct Scalars {
    unsigned long long ncand;
    unsigned long long nrec;
    unsigned long long nslots;   // call run: column-store slots (k_run_totals)
    unsigned long long nccs;
    unsigned long long log[16];
    int err;
    int dirty_over;          // normcounts: k_norm_quad left more positions to k_norm_dirty than a part of the list holds
    unsigned int nredo;      // normcounts: tiles k_norm_quad left to k_norm_tile
    int pad[21];             // 256 bytes: one aligned fill clears it
};
static_assert(sizeof(Scalars) == 256, "Scalars is cleared with one aligned fill");

// what upload_chunks made of a chunk list and the current reads
struct ChunkTables {
    int64_t n = 0, positions = 0, n_tiles = 0, npairs = 0, maxpairs = 0;   // maxpairs: the most reads under one chunk
};

// What a run keeps for its getter: the records on the host once they have been asked for (valid: h holds them), their
// number, the counters.  begin_run empties it, take_log and the run fill it, get_run_out serves it (below).
template <class Rec, int NLOG>
struct RunOut {
    std::vector<Rec> h;
    bool valid = false;
    int64_t n = 0, log[NLOG] = {};
    void begin() { valid = false; n = 0; std::fill(log, log + NLOG, (int64_t)0); }
};

// the column front's plan (front_plan, below)
struct ColumnFront {
    bool spec = false;
    int64_t nblk = 0, nwords = 0, marked = -1;   // marked: the marked positions (-1: on kept capacities, not known to the host)
    int idx_per = 1;                             // the column index: blocks per thread, workgroups
    unsigned idx_wgs = 1;
    size_t lead_bytes = 0;                       // bytes of the position bitmap the run uses
    size_t slot_cap = 0;                         // slots of the column store: kept, or (behind front_capture) counted
    int64_t rmask_cells = 0;                     // call run, proposals by rank: 16-bit cells of the mask (sized with the column store)
    PosIndex X{};
};

// what the host knows of a call run before anything of it is queued (call_plan, himut_call.hip); on kept capacities
// (spec) that is all of it, else ncap and nreserve come with the counts (call_candidates)
struct CallPlan {
    ChunkTables T;
    bool phase = false;
    bool spec = false;                           // nothing of the run waits for the host
    bool by_rank = false;                        // chunks in order: the mask is indexed by column rank (else by chunk cell)
    bool clear_all = false;                      // the mask or the tile counts are not known to hold zeros only
    int64_t n4 = 0, anyw = 0;                    // by cell: the mask in 16-byte pieces (8 positions each); in sweeps of 32 cells (a thread's)
    size_t mask_bytes = 0;
    unsigned mtiles = 1;                         // mask tiles: the workgroups of the emit (by rank: the column index's)
    size_t scan_tiles = 0, sort_tmp = 0;         // rocPRIM's temporary storage: the tile scan's, the candidate sort's
    int64_t ncap = 0, nreserve = 0;              // candidates: grid / scan extent, buffer capacity (records)
    ColumnFront F;
};

// The ordered event list of the indels and indelcal runs (indel_front_run, himut_indels.hip), one per run: the region
// tables, the keys and events before and behind the sort, the scalars block.
struct IndelEventList {
    DevBuf d_sstart, d_spmax, d_keys, d_keys2, d_vals, d_ev, d_ord, d_sorttmp, d_sc;
    int64_t cap_events = 0;                      // events kept from the list's previous run (0 = not known yet)
};

// What a pass over a site list keeps (sites_front / sites_back, himut_sites.hip): the sites, the records, the scalars.
struct SitesBufs {
    DevBuf d_pos, d_code, d_recs, d_sc;
    int64_t cap_slots = 0;                       // column-store slots kept from the previous pass (0 = not known yet)
};

// a call run whose host half is still to come (himut_run_begin / himut_run_end): what finish_run needs of it
struct PendingRun {
    bool active = false;
    CallPlan plan;
};

// The passes of a normcounts contig (do_normcounts, himut_norm.hip).  The callable run plans as a Tile pass: no lists.
enum class NormPass { First, MoreRoom, Tile };

// what the host knows of a normcounts pass -- or of a callable run, which takes the same front -- before anything of it
// is queued (norm_plan)
struct NormPlan {
    ChunkTables T;
    bool phase = false;
    bool work = false;                       // there are reads and chunks: without either no kernel is launched
    bool quad = false;                       // k_norm_quad's sweep with its two lists; else k_norm_tile for the whole contig
    size_t ntri = 0;                         // K^3: entries of one trinucleotide histogram
    int32_t maxspan = 1;                     // positions of the longest chunk
    int64_t q_per = 0, q_regions = 0;        // workgroup tiles of a chunk per XCD class; workgroups of k_norm_quad = list parts
    unsigned q_gx = 0, redo_cap = 0;         // k_norm_quad's workgroups per chunk; entries of the list of tiles
    int64_t n_tiles = 0, n_dirty = 0, nblk = 0;   // rows of the plan, entries of the list of positions, blocks of the window index
    const int64_t *d_toff = nullptr, *d_doff = nullptr;   // the layout table on the device (norm_layout)
    Reads R; Derived D; Chunks C; Phase H;   // the buffers' views, once all are reserved
    Scalars* sc = nullptr;
};

}  // namespace himut

struct himut_ctx {
    int device = 0;
    int n_cus = 256;
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;   // work that needs nothing from the cs decode runs here, beside it
    hipEvent_t ev[himut::EV_COUNT] = {};
    std::string err;
    int timing = 1;                          // himut_set_stage_timing: 0 total only, 1 + the column capture, 2 every stage
    himut_run_stats stats{};

    // ---- inputs every pipeline shares
    himut::Params params{};
    bool have_params = false, have_lut = false, have_reads = false;
    himut::DevBuf d_lut;
    // chunks (himut_set_chunks) and the device tables built for them (upload_chunks)
    std::vector<int32_t> cstart, cend;
    himut::DevBuf d_cstart, d_cend, d_maskoff, d_tileoff, d_sstart, d_sidx, d_spmax, d_rlo, d_rhi, d_pairoff, d_hint, d_crec, d_mtile;
    himut::DevBuf d_blkchunk;            // chunks in order: per 256-position block the first chunk that ends at or behind its
    int64_t n_blkchunk = 0;              // first tpos (k_mask_emit), for the blocks up to the last chunk's end
    std::vector<int32_t> up_cs, up_ce;   // the chunk list the device tables were built for
    bool tables_valid = false, chunks_in_order = false;
    int64_t up_positions = 0, up_tiles = 0, up_pairs = 0, up_maxpairs = 0;
    int64_t nhint = 0;
    std::vector<int64_t> maskoff, tileoff;
    // site sets (himut_set_site_set)
    himut::DevBuf d_pon, d_com, d_posbits;
    std::vector<uint64_t> h_pon, h_com;
    int64_t npon = 0, ncom = 0, nposbits = 0;
    // phase sets (himut_set_phase) and the reads' haplotypes (k_read_hap)
    bool have_phase = false;
    std::vector<int64_t> h_phoff;
    himut::DevBuf d_phoff, d_hpos, d_href, d_halt, d_hbit, d_hap;
    // reads (himut_push_reads or the ingest)
    int64_t n = 0, cs_bytes = 0, seq_bytes = 0, bq_bytes = 0, read_bases = 0;
    std::vector<int32_t> h_tstart, h_tend, h_prefmax;
    bool unique_qnames = true, any_longcs = false;
    himut::DevBuf d_tstart, d_tend, d_qstart, d_qlen, d_mapq, d_flag, d_qid, d_qoff, d_csoff, d_seq, d_bq, d_cs, d_prefmax;
    // derived by the read pass (alloc_derived)
    himut::DevBuf d_bqsum, d_nseg, d_nmis, d_nnsub, d_segs, d_mis, d_mq, d_meta, d_rflag, d_ccs;
    himut::DevBuf d_nonacgt;                 // per read: SEQ holds a base outside ATGC (k_flag_bases, once per batch)
    bool bases_flagged = false;              // d_nonacgt holds k_flag_bases' answer for the pushed reads
    himut::DevBuf d_winlo, d_winhi;
    int64_t win_nblk = 0;                    // d_winlo / d_winhi hold the read windows of the pushed reads for this many
                                             // 256-position blocks (0: not computed yet)
    // the decode's group plan (ensure_group_plan, himut_front.hip): per read whether it starts a group, the groups' first
    // reads, their number; the selection's scratch
    himut::DevBuf d_gflag, d_gfirst, d_gcount, d_gtmp;
    bool plan_valid = false;                 // d_gfirst / n_groups hold the plan of the pushed reads
    int64_t n_groups = 0;
    double plan_ms = 0;                      // device time of the plan's kernels
    int dbg_decode = 0;                      // himut_debug_decode (tests): 1 = every read a group of its own
    bool dbg_decode_on = false;              // ... was called: the decode counts its groups and keeps a copy of its bitmap
    himut::DevBuf d_dbgcnt, d_dbgbits;
    int64_t dbg_bits_words = 0;
    // the resident reference string (himut_set_reference)
    himut::DevBuf d_refseq;
    int64_t reflen = 0;
    uint8_t ref_cls[256] = {};
    int ref_K = 0;
    // the scalars block, on the device and its pinned landing zone on the host
    himut::DevBuf d_scalars;
    void* h_scalars = nullptr;
    size_t lead_clean_bytes = 0;      // bytes of the position bitmap (and the scalars) a run over the column front left empty for the next
    // context-wide scratch: any pass may take them for the length of the pass
    himut::DevBuf d_tmp, d_tmp2;
    // the device side of the process's pinned staging windows (size_pinned): the ingest's and the FASTA count's
    himut::DevBuf d_stage[2];
    hipEvent_t stage_copied[2] = {}, stage_parsed[2] = {};

    // ---- the call run (himut_call.hip); the column front's buffers (himut_front.hip: the bitmap, the block tables, the
    // column store) and the dense pile's (himut_pile.hip) are kept here too
    struct Call {
        himut::PendingRun pending;   // a run whose host half is still to come (himut_run_begin / himut_run_end)
        himut::DevBuf d_mask, d_recs, d_recs_out, d_keys, d_keys2, d_emit, d_pos, d_tilecnt, d_tileoff2, d_logpart;
        himut::DevBuf d_cands, d_cands2, d_blkslots, d_blkoff, d_blktab, d_colstore, d_posbits_c, d_posrank;
        himut::DevBuf d_dense_counts, d_dense_bqsum, d_tiles;   // himut_pile_counts
        // capacities the candidate / column buffers were last sized for: a run whose counts fit them goes
        // through without a host round trip in the middle (0 = not known yet)
        int64_t cap_cand = 0, cap_slots = 0;
        bool mask_clean = false;             // d_mask and d_tilecnt hold zeros only (a run's emit leaves them so, whichever way
                                             // the run indexed the mask: one buffer serves both)
        himut::RunOut<himut_record, 15> out;
    } call;

    // ---- normcounts (himut_norm.hip)
    struct Norm {
        himut::DevBuf d_refcode;             // per reference position: what the sweep wants to know about the letter (k_ref_codes)
        himut::DevBuf d_live, d_callable, d_dirty, d_dcount, d_redo, d_plan, d_plancnt, d_tri;
        himut::DevBuf d_lay;                 // the sweep's layout: the chunks' first plan rows, the parts' first list entries
        std::vector<int64_t> h_lay, h_swept;   // the table and the positions each workgroup sweeps, for the chunks below
        std::vector<int32_t> lay_cs, lay_ce;
        int64_t lay_room = 0, lay_dbg = 0;
        bool lay_ok = false;
        int dbg_sweep = 0, dbg_pool = 0;     // himut_debug_normcounts (tests)
        int64_t dbg_dirty_cap = 0;
        int64_t dirty_room = 0;              // entries of k_norm_dirty's list per NQ_WG_COLS swept positions an earlier pass needed
        std::vector<unsigned long long> h_tri;   // ccs[K^3], ref[K^3], log[16]
        bool have = false;
        int64_t cal_words = 0, cal_reads = 0;   // what the last completed pass's k_callable wrote (himut_debug_norm_callable)
    } norm;

    // ---- device-side BAM ingest (himut_ingest.hip)
    struct Ingest {
        void* pinned[2] = {nullptr, nullptr};
        size_t window = 0, bound = 0;
        bool sized = false;
        himut::DevBuf d_recoff[2], d_qidin[2], d_desc, d_sizes, d_offs, d_istate, d_tp;
        bool open = false, used[2] = {false, false};
        int64_t reads = 0, bases = 0, cs = 0;   // capacity the windows so far may need (upper bounds)
        // himut_ingest_derive_cs: the mode asked for, the mode of the open ingest; the CIGAR side array and its offsets
        // (they stand in for d_cs / d_csoff while the windows come in), the post-pass's lengths and refusals
        int derive = 0;
        bool derive_on = false;
        himut::DevBuf d_cig, d_cigoff, d_cslen, d_csbad, d_dstate;
        int64_t derive_res[3] = {0, 0, 0};      // himut_ingest_derive_result: derived, refused, bytes of text
        double derive_ms = 0;
    } ingest;

    // ---- the germline run (himut_germ.hip)
    struct Germ {
        himut::DevBuf d_refmask, d_nrefbits, d_recs, d_recs_out, d_wgcnt, d_logpart;
        // capacities kept from the previous germline run (0 = not known yet): marked positions, column-store slots
        int64_t cap_marked = 0, cap_slots = 0;
        himut::RunOut<himut_record, 12> out;
    } germ;

    // ---- the support run (himut_support.hip): buffers and scalars of its own, nothing of another run's is borrowed
    struct Support {
        himut::DevBuf d_pos, d_code, d_counts, d_rowoff, d_cursor, d_rows_in, d_rows, d_sc;
        std::vector<himut_support_row> h_rows;
        std::vector<int32_t> h_counts;       // n_sites x {cover, alt_reads}
        int64_t n_rows = 0, n_sites = 0;
    } support;

    // ---- the bqcal run (himut_bqcal.hip): buffers and scalars of its own, as the support run
    struct Bqcal {
        himut::DevBuf d_rstart, d_rend, d_tileoff, d_sstart, d_spmax, d_tiles, d_part, d_out, d_sc;
        int dbg_rb = 0;                      // himut_debug_bqcal (tests): rows per LDS batch, 0 = all there is room for
        int64_t out[2 * 256 + 12] = {};      // match, mismatch, log of the last run
    } bqcal;

    // ---- the callable run (himut_callmap.hip): the per-position map, the runs and the scan's scratch are its own; the
    // read pass in front of it is the normcounts run's and writes that run's read-pass buffers (norm.d_live, norm.d_callable)
    struct Callmap {
        himut::DevBuf d_mapoff, d_state, d_bases, d_blk, d_bnd, d_runs, d_sc;
        himut::RunOut<himut_callable_run, 14> out;   // the runs: the run itself copies them (valid when it completes)
        bool have = false;
        int64_t n_pos = 0;                   // swept positions of the last completed run
        // the geometry of that run, for the intervals run (himut_intervals.hip): a later himut_set_chunks changes nothing there
        std::vector<int32_t> g_cs, g_ce;
        int64_t g_reflen = 0;
        bool last_ok = false;                // the last himut_run_callable call completed
    } callmap;

    // ---- the intervals run (himut_intervals.hip): the callable run's map per interval; the intervals, the chunk copies,
    // the plan and the rows are its own
    struct Intervals {
        himut::DevBuf d_start, d_end, d_cs, d_ce, d_lo, d_hi, d_chunks, d_cnt, d_off, d_scantmp, d_rows;
        himut::RunOut<himut_interval_row, 1> out;
        bool have = false;
    } intervals;

    int64_t dbg_fasta_window = 0;            // himut_debug_fasta_window (tests): staging window bytes, 0 = default
    int dbg_spectra_wgs = 0;                 // himut_debug_spectra (tests): the most workgroups of k_id83 / k_dbs78 and of the
                                             // strand kernels (himut_strands.h), 0 = default
    int dbg_fit_wgs = 0, dbg_fit_lds = 0;    // himut_debug_fit (tests): the most workgroups of k_fit_resample / k_fit_em, the
                                             // LDS budget of a workgroup of k_fit_em in bytes; 0 = default

    // ---- the transcription-strand segment list of the resident string (himut_set_strands, himut_strands.hip):
    // himut_set_reference drops it
    struct Strands {
        himut::DevBuf d_start, d_mask;
        int64_t n = 0;                       // segments; 0 = no list
    } strands;

    // ---- the dbs run (himut_dbs.hip): behind the column front (the call run's bitmap, block tables and column store);
    // the keys, the records and the scalars are its own
    struct Dbs {
        himut::DevBuf d_keys, d_keys2, d_sorttmp, d_recs, d_recs_out, d_wgcnt, d_sc;
        // capacities kept from the previous dbs run (0 = not known yet): proposed keys, column-store slots
        int64_t cap_props = 0, cap_slots = 0;
        himut::RunOut<himut_dbs_record, 20> out;
    } dbs;

    // ---- the sites run (himut_sites.hip): over the column front (the call run's bitmap, block tables and column store);
    // the sites, the records and the scalars are its own
    struct Sites : himut::SitesBufs {
        himut::RunOut<himut_site_record, 20> out;
    } sites;

    // ---- the indels run (himut_indels.hip): behind the cs decode alone; the region tables, the events,
    // the records and the scalars are its own
    struct Indels {
        himut::IndelEventList ev;
        himut::DevBuf d_recs, d_recs_out, d_wgcnt;
        himut::DevBuf d_errtab;              // himut_set_indel_error_table: RUN_CELLS doubles of l_hit, then as many of l_err
        bool have_errtab = false;
        himut::RunOut<himut_indel_record, 13> out;
    } indels;

    // ---- the indelcal run (himut_indelcal.hip): behind the same ordered events (indel_front_run), in an event list, a
    // position bitmap and scalars of its own: no other run's getter loses what it serves
    struct Indelcal {
        himut::IndelEventList ev;
        himut::DevBuf d_bits;                // bit a: anchor a is variant
        himut::DevBuf d_blkflag;             // per 256-position block of the sweep: what the regions hold of it (k_indelcal_blocks)
        int dbg_wgs = 0;                     // himut_debug_indelcal (tests): workgroups of the sweep, its cells' budget; 0 = default
        int64_t dbg_budget = 0;
        int64_t table[128 * 10] = {}, log[14] = {};   // of the last run
    } indelcal;

    // ---- the sindels run (himut_sindels.hip): behind the same ordered events (indel_front_run) in an event list of its
    // own, with the reads' verdicts (k_sindel_reads), records and scalars of its own; it reads indels.d_errtab
    struct Sindels {
        himut::IndelEventList ev;
        himut::DevBuf d_verdict, d_recs, d_recs_out, d_wgcnt;
        himut::RunOut<himut_sindel_record, 20> out;
    } sindels;

    // ---- the haplotag run (himut_haplotag.hip): behind the cs decode alone; the hetSNP arrays, the rows, the tallies and
    // the scalars are its own, and so are the host copies its getter serves
    struct Haplotag {
        himut::DevBuf d_pos, d_ref, d_alt, d_bit, d_set, d_rows, d_snps, d_sc;
        std::vector<himut_haplotag_row> h_rows;
        std::vector<himut_haplotag_snp> h_snps;
        int64_t log[13] = {};
    } haplotag;

    // ---- the duplex run (himut_duplex.hip): over the column front with the bitmap filled from its own candidates, through
    // the sites run's pass (sites_front / sites_back) on buffers of its own; the mates, the reads' verdicts, the keys, the
    // tallies, the records and the scalars are its own too
    struct Duplex {
        himut::SitesBufs sites;              // d_recs: the candidates' site records, the first 64 bytes of the run's records
        himut::DevBuf d_mate, d_verdict, d_sstart, d_spmax, d_keys, d_keys2, d_uniq, d_nds, d_sorttmp, d_rletmp, d_tally, d_recs, d_sc;
        int64_t cap_keys = 0;                // keys kept from the previous duplex run (0 = not known yet)
        int64_t ss[12] = {};
        himut::RunOut<himut_duplex_record, 40> out;
    } duplex;
};

namespace himut {

inline int fail(himut_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

template <class F>
int guarded(himut_ctx* c, F f) {
    try {
        (void)hipGetLastError();   // an error some earlier call left behind is not this call's
        return f();
    } catch (const HipFail& h) {
        char buf[512];
        snprintf(buf, sizeof(buf), "HIP error %d (%s) at %s (%s:%d)", (int)h.e, hipGetErrorString(h.e), h.what, h.file, h.line);
        return fail(c, HIMUT_ERR_HIP, buf);
    } catch (const std::bad_alloc&) {
        return fail(c, HIMUT_ERR_NOMEM, "host allocation failed");
    } catch (...) {
        return fail(c, HIMUT_ERR_ARG, "unexpected C++ exception");
    }
}

// the first error bit the kernels set, as a return code and a message
int check_device_err(himut_ctx* c, int bits);

// What a run needs before it starts, checked in this order: the call run's parameters, the genotype table, reads, a
// region list, the reference, and last (NEED_SPANS) that no region has start > end.
enum : unsigned { NEED_PARAMS = 1, NEED_LUT = 2, NEED_READS = 4, NEED_REGIONS = 8, NEED_SPANS = 16, NEED_REFERENCE = 32 };
int check_run_inputs(himut_ctx* c, unsigned needs);

// what the call run needs before it starts (normcounts: and the reference)
int check_scan_inputs(himut_ctx* c, bool need_reference = false);

// The site list of the support and sites runs, validated (1-based and non-decreasing; ref and alt two different letters
// of ATGC), as one code per site: (ref << 2) | alt.  who: the caller's name, for the messages.
int encode_sites(himut_ctx* c, const char* who, const int32_t* pos1, const uint8_t* ref, const uint8_t* alt, int64_t n_sites,
                 std::vector<uint8_t>* code);

// stage events cost a barrier packet each (a few microseconds of queue time): only the ones asked for are recorded
inline void stage_event(himut_ctx* c, int ev, int level, hipStream_t st) {
    if (c->timing >= level) HCHECK(hipEventRecord(c->ev[ev], st));
}

// milliseconds between two of the context's stage events (0 when one was not recorded)
inline double elapsed_ms(himut_ctx* c, int a, int b) {
    float f = 0;
    (void)hipEventElapsedTime(&f, c->ev[a], c->ev[b]);
    return (double)f;
}

// new reads: the chunk tables, the read windows, the base flags, the decode's group plan and the records on the host are stale
inline void forget_reads(himut_ctx* c) {
    c->tables_valid = false; c->win_nblk = 0; c->bases_flagged = false; c->plan_valid = false; c->call.out.valid = false;
}

inline unsigned blocks_for(int64_t n, int per) { return (unsigned)std::max<int64_t>(1, (n + per - 1) / per); }

// the scalars for a pass other than the call run: the next call run clears them (and its bitmap) first
inline Scalars* borrow_scalars(himut_ctx* c) {
    c->lead_clean_bytes = 0;
    return c->d_scalars.as<Scalars>();
}

inline Reads make_reads(himut_ctx* c) {
    Reads R;
    R.n = c->n;
    R.tstart = c->d_tstart.as<int32_t>(); R.tend = c->d_tend.as<int32_t>(); R.qstart = c->d_qstart.as<int32_t>();
    R.qlen = c->d_qlen.as<int32_t>(); R.mapq = c->d_mapq.as<uint8_t>(); R.flag = c->d_flag.as<uint16_t>();
    R.qid = c->d_qid.as<int32_t>(); R.qoff = c->d_qoff.as<int64_t>(); R.cs_off = c->d_csoff.as<int64_t>();
    R.seq = c->d_seq.as<uint8_t>(); R.bq = c->d_bq.as<uint8_t>(); R.cs = c->d_cs.as<uint8_t>();
    R.prefmax_tend = c->d_prefmax.as<int32_t>();
    R.nonacgt = c->d_nonacgt.as<uint8_t>();
    return R;
}

inline Derived make_derived(himut_ctx* c) {
    Derived D;
    D.bqsum = c->d_bqsum.as<uint32_t>(); D.nseg = c->d_nseg.as<int32_t>(); D.nmis = c->d_nmis.as<int32_t>();
    D.segs = c->d_segs.as<Seg>(); D.mis = c->d_mis.as<int32_t>(); D.mq = c->d_mq.as<uint32_t>();
    D.rflag = c->d_rflag.as<uint8_t>(); D.meta = c->d_meta.as<ReadMeta>(); D.nnsub = c->d_nnsub.as<int32_t>();
    return D;
}

inline Chunks make_chunks(himut_ctx* c, int64_t n) {
    Chunks C;
    C.n = n;
    C.rec = c->d_crec.as<ChunkRec>(); C.mtile = c->d_mtile.as<MaskTile>();
    C.start = c->d_cstart.as<int32_t>(); C.end = c->d_cend.as<int32_t>();
    C.maskoff = c->d_maskoff.as<int64_t>();
    C.s_start = c->d_sstart.as<int32_t>(); C.s_idx = c->d_sidx.as<int32_t>(); C.s_pmaxend = c->d_spmax.as<int32_t>();
    C.rlo = c->d_rlo.as<int64_t>(); C.rhi = c->d_rhi.as<int64_t>(); C.pairoff = c->d_pairoff.as<int64_t>();
    C.hint = c->d_hint.as<int32_t>(); C.nhint = c->nhint;
    return C;
}

inline Phase make_phase(himut_ctx* c) {
    Phase H;
    H.off = c->d_phoff.as<int64_t>(); H.hpos = c->d_hpos.as<int32_t>(); H.href = c->d_href.as<uint8_t>();
    H.halt = c->d_halt.as<uint8_t>(); H.hbit = c->d_hbit.as<uint8_t>(); H.hap = c->d_hap.as<uint8_t>();
    return H;
}

// the panel of normals, the common SNPs and the bitmap of their positions (himut_set_site_set)
inline SiteSets site_sets(himut_ctx* c) {
    SiteSets S;
    S.pon = c->d_pon.as<uint64_t>(); S.npon = c->npon; S.com = c->d_com.as<uint64_t>(); S.ncom = c->ncom;
    S.posbits = c->d_posbits.as<uint32_t>(); S.nposbits = c->nposbits;
    return S;
}

// Uploads the chunk tables for the given chunk list and the current reads.
ChunkTables upload_chunks(himut_ctx* c, const std::vector<int32_t>& cs, const std::vector<int32_t>& ce);
// The regions (cs[k], ce[k]) by start -- a stable sort: regions of equal start keep the list's order -- as sstart[j], the
// j-th smallest start, and spmax[j], the maximum of the ends of the first j + 1 of them (from INT32_MIN); sidx[j], where
// asked for, is the j-th region's place in the list.  What a kernel's in-region look-up walks (chunk tables, k_bqcal_bases,
// k_indel_events).
void sorted_regions(const std::vector<int32_t>& cs, const std::vector<int32_t>& ce, std::vector<int32_t>* sstart,
                    std::vector<int32_t>* spmax, std::vector<int32_t>* sidx = nullptr);

// ---- the normcounts front (himut_norm.hip), which the callable run takes too: the sizes and every buffer of a pass
// (norm_plan, which lays the sweep's scratch out with norm_layout), EV_START .. EV_EMIT (norm_read_pass: the decode,
// the read filters, the callable bits, the reads' haplotypes, the window index) and the sweep kernels' argument block
struct NormArgs;
void norm_layout(himut_ctx* c, NormPlan* P, int64_t dbg_cap);
NormPlan norm_plan(himut_ctx* c, const ChunkTables& T, NormPass pass);
void norm_read_pass(himut_ctx* c, const NormPlan& P);
NormArgs norm_args(himut_ctx* c, const NormPlan& P, const uint8_t* alt_order, int non_human);

// ---- the read pass (himut_front.hip)
void alloc_derived(himut_ctx* c);
// once per pushed batch: which reads hold a base outside ATGC somewhere (on `st`, in front of whatever looks at the flags)
void flag_bases_once(himut_ctx* c, hipStream_t st);
// the cs decode; P: the parameter block it runs under (null: the call run's, himut_set_params)
void run_parse_stage(himut_ctx* c, const Reads& R, const Derived& D, Scalars* sc, const Params* P = nullptr);
void launch_window_index(himut_ctx* c, const Reads& R, int64_t nblk, hipStream_t st);
void launch_read_hap(himut_ctx* c, const Reads& R, const Derived& D, const Chunks& C, const Phase& H, const ChunkTables& T, Scalars* sc);
void launch_count_flags(himut_ctx* c, Scalars* sc);

// ---- the column front (himut_front.hip): what the call, germline, dbs and sites runs have in common, in steps on one
// ColumnFront.  What a run does before, between and behind them is its own (the call run: k_read_hap between the decode
// and the capture; both: their kernels between the capture and the tail).  The front alone owns lead_clean_bytes and
// win_nblk.
//   front_plan     the sizes, and every buffer whose size the host knows up front: before anything of the run is queued
//                  (DevBuf::reserve drains the device when it grows).  spec: the column store keeps `kept_slots` slots
//                  and nothing in the front waits for the host.  span_chunks: the bitmap spans the chunks as well as
//                  the reads (false: the reads alone -- a run without regions).
//   front_decode   EV_START .. EV_PARSE: the cs decode with the bitmap gate under P; clear_mask: the call run's mask and
//                  tile counts are cleared beside it.
//   front_capture  .. EV_INDEX .. EV_GATHER: the column index and k_stream_capture; unless spec the host sizes the
//                  column store in between (F->slot_cap, F->marked).  proposals: the call run's, into its mask and tile
//                  counts; by rank the mask is sized with the column store (F->rmask_cells).
//   front_totals   behind the capture, for a run that keeps scalars of its own (dbs, sites): the marked positions and the
//                  column-store slots of the run into sc[i_marked] and sc[i_slots], which the host compares with the
//                  kept capacities.
//   front_tail     EV_FINAL, the scalars to their pinned block, EV_COPIED, and behind the copy the fills that leave the
//                  scalars and the bitmap empty for the next run over the front (the host does not wait for these).
//   front_tail_wait  the host's side: waits for EV_COPIED (not for the stream), checks the device's error word, and
//                  notes what the fills leave empty.  The scalars are in c->h_scalars then.
//   front_stats    the run's figures and stage times (EVAL_STAGES: the table of the germline, dbs and sites runs);
//                  kept_slot_cap: the column-store capacity a run leaves for the next one of its kind.
ColumnFront front_plan(himut_ctx* c, bool spec, int64_t kept_slots, bool span_chunks = true);
void front_decode(himut_ctx* c, const ColumnFront& F, const Params& P, bool clear_mask);
enum class Proposals { none, by_cell, by_rank };
int front_capture(himut_ctx* c, ColumnFront* F, const Chunks& C, const Phase& H, const Params& P, Proposals proposals);
// bytes of a mask by rank for a column store of slot_cap slots and nchunks chunks: the marked positions are at most the slots
inline size_t rank_mask_bytes(size_t slot_cap, int64_t nchunks) { return (slot_cap + (size_t)nchunks) * 2 + 64; }
void front_totals(himut_ctx* c, const ColumnFront& F, unsigned long long* sc, int i_marked, int i_slots);
void front_tail(himut_ctx* c, const ColumnFront& F);
int front_tail_wait(himut_ctx* c, const ColumnFront& F);

// The figures of a run over the front into c->stats (zeroed when the run began): the total, the capture from level 1,
// from level 2 the stages of the run's own table (a stage time is the span between two of the context's events).
struct StageSpan {
    double himut_run_stats::*ms;
    int from, to;
};
void front_stats(himut_ctx* c, const StageSpan* stages, size_t n_stages, int64_t positions, int64_t n_candidates, int64_t n_records,
                 int64_t column_slots);
// the stages of a run with one evaluation between the capture and the tail (germline, dbs, sites)
inline const StageSpan EVAL_STAGES[] = {{&himut_run_stats::ms_parse, EV_START, EV_PARSE}, {&himut_run_stats::ms_index, EV_PARSE, EV_INDEX},
                                        {&himut_run_stats::ms_eval, EV_GATHER, EV_SWEEP}, {&himut_run_stats::ms_finalize, EV_SWEEP, EV_FINAL}};
constexpr size_t N_EVAL_STAGES = sizeof(EVAL_STAGES) / sizeof(EVAL_STAGES[0]);
// the column-store slots a run that sized the store for slot_cap keeps for the runs that follow: 25 % of headroom
inline int64_t kept_slot_cap(size_t slot_cap) { return (int64_t)(slot_cap + slot_cap / 4 + 4096); }

// ---- the pass over a site list (himut_sites.hip), in two steps on one SitesFront, for the sites run and for a run whose
// sites come from the reads (duplex: its kernels run between the two, on the decoded reads).
//   sites_front    front_plan and front_decode under `decode`, which must keep every read out of the bitmap gate (closed
//                  query-length limits): EV_START .. EV_PARSE
//   sites_back     the n_sites sites of B.d_pos / B.d_code (device arrays, 1-based positions non-decreasing, ref << 2 | alt):
//                  their bits, the capture, k_sites_eval into B.d_recs, the front's tail; *overflow: the column slots did
//                  not fit the kept capacity and nothing of `out` is valid (run_repeating)
struct SitesFront {
    ColumnFront F;
    Params decode;
    bool spec = false;
};
struct SitesTotals {
    int64_t log[20] = {};                        // himut_get_sites' counters
    int64_t nslots = 0;
};
SitesFront sites_front(himut_ctx* c, SitesBufs& B, const Params& decode, bool allow_spec);
int sites_back(himut_ctx* c, SitesBufs& B, SitesFront& SF, int64_t n_sites, bool* overflow, SitesTotals* out);

// A run on kept capacities and its repeat: once(kept, &overflow) sets overflow if a count did not fit what an earlier
// run left; then forget() drops the capacities, the run is made again with exact sizes, and the stats say so.
template <class Once, class Forget>
int run_repeating(himut_ctx* c, Once once, Forget forget) {
    bool overflow = false;
    int rc = once(true, &overflow);
    if (rc == HIMUT_OK && overflow) {
        forget();
        rc = once(false, &overflow);
        c->stats.reran = 1;
    }
    return rc;
}

// ---- the counted key list of the dbs and indels runs: a kernel appends 64-bit keys to a list and counts in a device
// word how many it wanted to append (it writes none past the capacity it is given), rocPRIM sorts the list, and a grid
// sized by the count works on it.
// one 64-bit word of device memory (the host waits for the stream)
inline int64_t read_word(himut_ctx* c, const unsigned long long* d) {
    unsigned long long n = 0;
    HCHECK(hipMemcpyAsync(&n, d, 8, hipMemcpyDeviceToHost, c->stream));
    HCHECK(hipStreamSynchronize(c->stream));
    return (int64_t)n;
}

struct KeyCount {
    int64_t n, cap;     // the keys the kernel wanted to append; the capacity it was given
    bool over;          // n > cap: only a run on a kept capacity can get here (the caller runs again with exact sizes)
};

// launch(cap) queues the appending kernel behind a cleared count word d_count; reserve(cap) sizes every buffer that
// depends on the capacity (before launch(cap) is queued: DevBuf::reserve drains the device when it grows).  spec: the
// buffers hold kept_cap keys already and the host waits once, for the count.  Otherwise the count first (nothing is
// written with no capacity), then the buffers with 25 % of headroom for the runs that follow, then the keys: two waits.
template <class Launch, class Reserve>
KeyCount count_keys(himut_ctx* c, bool spec, int64_t kept_cap, const unsigned long long* d_count, Launch launch, Reserve reserve) {
    int64_t cap = kept_cap;
    if (!spec) {
        launch((int64_t)0);
        const int64_t n = read_word(c, d_count);
        cap = n + n / 4 + 1024;
        reserve(cap);
    }
    launch(cap);
    const int64_t n = read_word(c, d_count);
    return {n, cap, n > cap};
}

// rocPRIM's two calls: sort(nullptr, bytes) says how much temporary storage the sort wants, d_tmp is reserved for it, and
// with `run` sort(d_tmp.p, bytes) is queued (without: the sizing alone, for a capacity; the sort of fewer keys may want
// more room than the sort of the capacity, so a run sizes again for its count).
template <class Sort>
void sort_with_tmp(DevBuf& d_tmp, bool run, Sort sort) {
    size_t bytes = 0;
    HCHECK(sort(nullptr, bytes));
    d_tmp.reserve(bytes + 256);
    if (run) HCHECK(sort(d_tmp.p, bytes));
}

// the first lines of a run: the device, an empty result block, empty stats
template <class Out>
void begin_run(himut_ctx* c, Out& out) {
    HCHECK(hipSetDevice(c->device));
    out.begin();
    memset(&c->stats, 0, sizeof(c->stats));
}

// the run's counters from the scalars the host read back (64-bit words of the Scalars block, or a run's own words)
template <class Rec, int NLOG, class Word>
void take_log(RunOut<Rec, NLOG>& out, const Word* words) { for (int k = 0; k < NLOG; k++) out.log[k] = (int64_t)words[k]; }

// the body of a run's getter: the records, copied from d_recs when first asked for, their number, the counters (log may be null)
template <class Rec, int NLOG>
int get_run_out(himut_ctx* c, RunOut<Rec, NLOG>& out, const DevBuf& d_recs, const Rec** records, int64_t* n, int64_t* log) {
    if (!out.valid) {
        HCHECK(hipSetDevice(c->device));
        out.h.resize((size_t)out.n);
        if (out.n) HCHECK(hipMemcpyAsync(out.h.data(), d_recs.p, (size_t)out.n * sizeof(Rec), hipMemcpyDeviceToHost, c->stream));
        HCHECK(hipStreamSynchronize(c->stream));
        out.valid = true;
    }
    *records = out.h.data(); *n = out.n;
    if (log) std::copy(out.log, out.log + NLOG, log);
    return HIMUT_OK;
}

// the decode's parameter block for a run that takes every read of the pile: min_mapq, the other gates open (no
// query-length limits, every identity passes)
inline Params open_gate_params(const himut_ctx* c, int32_t min_mapq) {
    Params P{};
    P.p.min_mapq = min_mapq;
    P.p.qlen_lower_limit = -1; P.p.qlen_upper_limit = INT_MAX;
    P.p.min_sequence_identity = -1.0;
    P.unique_qnames = c->unique_qnames ? 1 : 0;
    return P;
}

// The process's two pinned staging windows (pinning 128 MB takes tens of milliseconds; a call makes one context per
// contig): one context holds them at a time, from claim_pinned to release_pinned.  claim_pinned fails (nothing taken)
// while another context holds them, or c itself unless `own_ok`.  size_pinned, for the holder: the windows at least
// `bytes` each (allocated with `flags`; returns whether they had to be allocated again) into `host`, with c's device
// staging buffers and copy / parse events.
bool claim_pinned(himut_ctx* c, bool own_ok);
bool size_pinned(himut_ctx* c, size_t bytes, unsigned flags, void* host[2]);
void release_pinned(himut_ctx* c);

}  // namespace himut
