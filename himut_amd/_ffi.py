"""ctypes binding of libhimut_hip.so (include/himut_hip.h).

The HIP extension is the only compute path: if the library cannot be loaded
the import of this module's ``lib()`` raises -- there is no CPU fallback.
"""
import ctypes
import os
import sys

import numpy as np

from . import build
from .readbatch import READ_ARRAYS, ReadBatch, read_arrays

STATUS_NAMES = ["PASS", "LowBQ", "LowGQ", "IndelSite", "HetSite", "HetAltSite", "HomAltSite", "ComSnp",
                "PanelOfNormal", "LowDepth", "HighDepth", "Unphased"]

RECORD_DTYPE = np.dtype([("tpos", "<i4"), ("chunk", "<i4"), ("phase_set", "<i4"), ("gq", "<i4"), ("ref", "u1"),
                         ("alt", "u1"), ("gt0", "u1"), ("gt1", "u1"), ("status", "u1"), ("gt_state", "u1"),
                         ("flags", "u1"), ("pad", "u1"), ("counts", "<u4", (6,)), ("bqsum", "<u4", (4,))])
assert RECORD_DTYPE.itemsize == 64          # himut_record

# himut_support_row (include/himut_hip.h): one (site, supporting read)
SUPPORT_ROW_DTYPE = np.dtype([("site", "<i4"), ("read", "<i4"), ("qid", "<i4"), ("tstart", "<i4"), ("tend", "<i4"),
                              ("qlen", "<i4"), ("flag", "<u2"), ("mapq", "u1"), ("bq", "u1"), ("qpos", "<i4"),
                              ("bq_sum", "<u4"), ("n_sub", "<i4"), ("n_indel", "<i4"), ("window_mismatches", "<i4")])
assert SUPPORT_ROW_DTYPE.itemsize == 48


# himut_dbs_record (include/himut_hip.h): one doublet base substitution
DBS_RECORD_DTYPE = np.dtype([("tpos", "<i4"), ("gq", "<i4"), ("ref", "u1", (2,)), ("alt", "u1", (2,)), ("status", "u1"),
                             ("half_status", "u1", (2,)), ("pad0", "u1"), ("gt_state", "u1", (2,)), ("gt", "u1", (2, 2)),
                             ("pad1", "u1", (2,)), ("half_gq", "<i4", (2,)), ("counts", "<u4", (2, 6)),
                             ("alt_bqsum", "<u4", (2,)), ("both_alt", "<u4"), ("both_ref", "<u4"), ("one_alt", "<u4"),
                             ("n_proposers", "<u4"), ("pad2", "<u4", (2,))])
assert DBS_RECORD_DTYPE.itemsize == 112

# himut_site_record (include/himut_hip.h): one site of a list genotyped on this sample's pile
SITE_RECORD_DTYPE = np.dtype([("site", "<i4"), ("tpos", "<i4"), ("ref", "u1"), ("alt", "u1"), ("status", "u1"),
                              ("gt_state", "u1"), ("gt", "u1", (2,)), ("pad", "u1", (2,)), ("gq", "<i4"),
                              ("counts", "<u4", (6,)), ("alt_bqsum", "<u4"), ("ref_bqsum", "<u4"), ("alt_hi", "<u4"),
                              ("alt_mq", "<u4"), ("reserved", "<u4")])
assert SITE_RECORD_DTYPE.itemsize == 64
# the statuses of a site record: the FILTER values and the two only the sites run gives (HIMUT_ST_GERMLINE, HIMUT_ST_NOCOV)
SITE_STATUS_NAMES = STATUS_NAMES + ["Germline", "NoCoverage"]

# himut_indel_record (include/himut_hip.h): one short insertion or deletion allele
INDEL_RECORD_DTYPE = np.dtype([("anchor", "<i4"), ("len", "<i4"), ("type", "u1"), ("status", "u1"), ("gt_state", "u1"),
                               ("pad0", "u1"), ("gq", "<i4"), ("dp", "<u4"), ("n_alt", "<u4"), ("n_other", "<u4"),
                               ("pad1", "<u4"), ("bases", "u1", (16,)), ("reserved", "<u4", (4,))])
assert INDEL_RECORD_DTYPE.itemsize == 64
INDEL_LOG_NAMES = ("events", "alleles", "num_edge", "num_long", "num_nbase", "num_dup", "homref", "het", "homalt", "PASS",
                   "LowGQ", "LowDepth", "HighDepth")

# himut_sindel_record (include/himut_hip.h): one somatic indel candidate; himut_indel_record's fields at its offsets
SINDEL_RECORD_DTYPE = np.dtype([("anchor", "<i4"), ("len", "<i4"), ("type", "u1"), ("status", "u1"), ("gt_state", "u1"),
                                ("pad0", "u1"), ("gq", "<i4"), ("dp", "<u4"), ("n_alt", "<u4"), ("n_other", "<u4"),
                                ("pad1", "<u4"), ("bases", "u1", (16,)), ("n_prop", "<u4"), ("run_base", "u1"),
                                ("run_len", "u1"), ("class_col", "u1"), ("pad2", "u1"), ("reserved", "<u4", (2,))])
assert SINDEL_RECORD_DTYPE.itemsize == 64
SINDEL_LOG_NAMES = ("events", "num_edge", "num_long", "num_nbase", "pile_reads", "proposing_reads", "events_proposing_reads",
                    "num_trim", "num_window", "num_lowbq", "proposing_events", "candidates", "num_germ_het",
                    "num_germ_homalt", "IndelSite", "Repeat", "LowGQ", "LowDepth", "HighDepth", "PASS")
ST_REPEAT = 14                              # HIMUT_ST_REPEAT
SINDEL_STATUS_NAMES = {0: "PASS", 2: "LowGQ", 3: "IndelSite", 9: "LowDepth", 10: "HighDepth", ST_REPEAT: "Repeat"}

# himut_callable_run (include/himut_hip.h): a stretch of equal state within one chunk, 0-based and half open
CALLABLE_RUN_DTYPE = np.dtype([("chunk", "<i4"), ("start", "<i4"), ("end", "<i4"), ("state", "<i4"), ("bases", "<i8")])
assert CALLABLE_RUN_DTYPE.itemsize == 24
# the states of the callable map (HIMUT_CM_*: the rows of norm.log, 0 and 1 for the positions that add to none)
CALLABLE_STATES = {0: "NON_ACGT", 1: "NO_BASE", 2: "UNPHASED", 3: "HET", 4: "HETALT", 5: "HOMALT", 7: "INDEL",
                   8: "HIGH_DEPTH", 9: "ALLELE_BALANCE", 10: "LOW_GQ", 11: "PON", 12: "COMMON_SNP", 13: "CALLABLE"}
CALLMAP_TILE, CALLMAP_BLOCK = 256, 2048     # HIMUT_CALLMAP_TILE, HIMUT_CALLMAP_BLOCK

# himut_interval_row (include/himut_hip.h): the callable run's map inside one interval; 128 int64
INTERVAL_ROW_DTYPE = np.dtype([("entries", "<i8"), ("positions", "<i8", (14,)), ("bases", "<i8", (14,)),
                               ("all_tri", "<i8", (33,)), ("ref_tri", "<i8", (33,)), ("ccs_tri", "<i8", (33,))])
assert INTERVAL_ROW_DTYPE.itemsize == 1024
# the 33 trinucleotide classes of a row: first * 8 + (centre == "T") * 4 + last with A0 C1 G2 T3, then every other key
INTERVAL_TRI_NAMES = tuple(a + m + b for a in "ACGT" for m in "CT" for b in "ACGT") + ("other",)

# himut_haplotag_row, himut_haplotag_snp (include/himut_hip.h): one per read, one per phased hetSNP
HAPLOTAG_ROW_DTYPE = np.dtype([("read", "<i4"), ("set", "<i4"), ("n0", "<u4"), ("n1", "<u4"), ("n_other", "<u4"),
                               ("n_del", "<u4"), ("n_lowbq", "<u4"), ("n_sets", "<u2"), ("hap", "u1"), ("status", "u1")])
HAPLOTAG_SNP_DTYPE = np.dtype([(k, "<u4") for k in ("n_ref", "n_alt", "n_other", "n_del", "n_lowbq", "agree", "disagree",
                                                    "pad")])
assert HAPLOTAG_ROW_DTYPE.itemsize == 32 and HAPLOTAG_SNP_DTYPE.itemsize == 32
# the statuses of a row (HIMUT_HT_*) and the thirteen counters
HAPLOTAG_STATUS_NAMES = ("Assigned", "NotInPile", "NoSnp", "NoVote", "LowSupport", "Conflict")
HAPLOTAG_LOG_NAMES = ("reads", "pile", "hap0", "hap1", "NoSnp", "NoVote", "LowSupport", "Conflict", "multi_set", "votes",
                      "other", "del", "lowbq")

# himut_duplex_record (include/himut_hip.h): himut_site_record's fields at their offsets, then the three counts
DUPLEX_RECORD_DTYPE = np.dtype(SITE_RECORD_DTYPE.descr + [("n_ds", "<u4"), ("n_ss", "<u4"), ("n_alt_unpaired", "<u4"),
                                                          ("reserved2", "<u4")])
assert DUPLEX_RECORD_DTYPE.itemsize == 80
# the forty counters of himut_get_duplex and the twelve classes of its single-strand spectrum
DUPLEX_LOG_NAMES = ("reads", "pile_reads", "proposing_reads", "pairs", "pairs_in_play", "pairs_notpile", "pairs_identity",
                    "pairs_lowqv", "pairs_qlen", "events", "num_trim", "num_window", "num_lowbq", "nocover", "del", "lowbq",
                    "trim", "concordant", "single", "other", "num_mate_window", "ds_events", "ds_events_in_chunk",
                    "ss_events_in_chunk", "ds_bases", "ds_pairs_overlap", "candidates", "Germline", "HetSite", "HetAltSite",
                    "HomAltSite", "IndelSite", "LowGQ", "LowBQ", "PanelOfNormal", "ComSnp", "LowDepth", "HighDepth", "PASS",
                    "reserved")
DUPLEX_SS_CLASSES = tuple(a + ">" + b for a in "ACGT" for b in "ACGT" if a != b)


class Params(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in (
        "min_qv", "min_mapq", "qlen_lower_limit", "qlen_upper_limit", "min_gq", "min_bq", "max_mismatch_count",
        "mismatch_window_size", "md_threshold", "min_ref_count", "min_alt_count", "min_hap_count", "phase",
        "reserved")] + [("min_sequence_identity", ctypes.c_double), ("min_trim", ctypes.c_double)]


class ReadBatchStruct(ctypes.Structure):
    _fields_ = [("n_reads", ctypes.c_int64)] + [(k, ctypes.c_void_p) for k, _ in READ_ARRAYS] + [
        ("seq_bytes", ctypes.c_int64), ("bq_bytes", ctypes.c_int64), ("cs_bytes", ctypes.c_int64)]

    @classmethod
    def of(cls, n, arrays):
        """Over the caller's arrays (name -> array, contiguous, of the READ_ARRAYS types): they must outlive the call."""
        return cls(n, *[_ptr(arrays[k]) for k, _ in READ_ARRAYS], *[int(arrays[k].shape[0]) for k in ("seq", "bq", "cs")])


# what himut_debug_read_pass copies out (himut_device.h: Seg, ReadMeta)
SEG_DTYPE = np.dtype([("t0", "<i4"), ("q0", "<i4"), ("len", "<i4"), ("flags", "<u4")])
READ_META_DTYPE = np.dtype([("tstart", "<i4"), ("tend", "<i4"), ("nseg", "<i4"), ("flags", "<u4"), ("segbase", "<i8"),
                            ("qoff", "<i8")])


class RunStats(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ("ms_total", "ms_parse", "ms_bqsum", "ms_hap", "ms_emit", "ms_index",
                                               "ms_capture", "ms_eval", "ms_finalize")] + \
               [(k, ctypes.c_int64) for k in ("n_reads", "read_bases", "positions", "n_unique_positions", "n_candidates",
                                              "n_records", "column_slots", "reran")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class GermlineParams(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("min_mapq", "min_gq", "min_bq", "min_ref_count", "min_alt_count",
                                              "md_threshold", "report_homref", "reserved")]


class SupportParams(ctypes.Structure):
    _fields_ = [("min_mapq", ctypes.c_int32), ("mismatch_window_size", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2)]


class BqcalParams(ctypes.Structure):
    _fields_ = [("min_mapq", ctypes.c_int32), ("min_gq", ctypes.c_int32), ("md_threshold", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 5)]


class IndelParams(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("min_mapq", "min_gq", "min_ref_count", "min_alt_count", "md_threshold",
                                              "max_len", "report_homref", "reserved")] + \
               [(k, ctypes.c_double) for k in ("l_hit", "l_err", "l_half")] + [("prior", ctypes.c_double * 3)]


def indel_logs(indel_error, germline_indel_prior):
    """The six doubles of himut_indel_params, computed here with math.log10 (the GtLut precedent): l_hit, l_err, l_half,
    then the log priors of homref, het and hom-alt."""
    import math
    e, pi = float(indel_error), float(germline_indel_prior)
    if not (0.0 < e < 1.0) or not (0.0 < pi < 2.0 / 3.0):
        raise ValueError("indel_error must lie in (0, 1) and germline_indel_prior in (0, 2/3)")
    return (math.log10(1 - e), math.log10(e), math.log10(0.5), math.log10(1 - 1.5 * pi), math.log10(pi),
            math.log10(pi / 2))


class SindelParams(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("min_mapq", "min_gq", "min_ref_count", "min_alt_count", "md_threshold",
                                              "max_len", "max_run", "min_qv")] + \
               [(k, ctypes.c_double) for k in ("l_hit", "l_err", "l_half")] + [("prior", ctypes.c_double * 3)] + \
               [(k, ctypes.c_int32) for k in ("qlen_lower_limit", "qlen_upper_limit", "min_bq", "mismatch_window_size",
                                              "max_mismatch_count", "reserved")] + \
               [("min_sequence_identity", ctypes.c_double), ("min_trim", ctypes.c_double)]


assert ctypes.sizeof(SindelParams) == 120   # himut_sindel_params


class IndelcalParams(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("min_mapq", "max_len", "min_alt_count", "vaf_permille")] + \
               [("reserved", ctypes.c_int32 * 4)]


# himut_run_indelcal (include/himut_hip.h): the table's shape and names, the fourteen counters
INDELCAL_CLASSES, INDELCAL_EVENT_COLUMNS = 128, 7
INDELCAL_COLUMNS = ("runs", "excluded", "spans", "del1", "del2", "del3p", "ins1", "ins2", "ins3p", "other")
INDELCAL_LOG_NAMES = ("events", "num_edge", "num_long", "num_nbase", "anchors", "variant_anchors", "events_variant",
                      "num_offrun", "num_partial", "events_counted", "runs", "runs_excluded", "runs_long", "spans")
INDEL_ERROR_CELLS = INDELCAL_CLASSES * INDELCAL_EVENT_COLUMNS       # HIMUT_INDEL_ERROR_CELLS


class HaplotagParams(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("min_mapq", "min_bq", "min_snps", "min_agree_permille")] + \
               [("reserved", ctypes.c_int32 * 4)]


class DuplexParams(ctypes.Structure):
    _fields_ = [("reserved", ctypes.c_int32 * 8)]


assert ctypes.sizeof(DuplexParams) == 32    # himut_duplex_params


class IngestResult(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int64) for k in ("n_reads", "bases_padded", "cs_bytes", "read_bases", "n_missing_cs",
                                              "n_unsorted", "n_malformed")]


# the device library's C ABI (include/himut_hip.h): name -> (restype, argtypes)
_I, _I32, _I64, _P, _S = ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_char_p
_PP, _PI64 = ctypes.POINTER(_P), ctypes.POINTER(_I64)
_ABI = {
    "himut_abi_version": (_I, []),
    "himut_create": (_I, [_I, _PP]),
    "himut_destroy": (None, [_P]),
    "himut_last_error": (_S, [_P]),
    "himut_set_params": (_I, [_P, ctypes.POINTER(Params)]),
    "himut_set_gt_lut": (_I, [_P, _P, _P, _P, _I, _P]),
    "himut_set_chunks": (_I, [_P, _P, _P, _I64]),
    "himut_set_site_set": (_I, [_P, _I, _P, _I64]),
    "himut_set_phase": (_I, [_P] * 6 + [_I64]),
    "himut_push_reads": (_I, [_P, ctypes.POINTER(ReadBatchStruct)]),
    "himut_run": (_I, [_P]),
    "himut_run_begin": (_I, [_P]),
    "himut_run_end": (_I, [_P]),
    "himut_get_records": (_I, [_P, _PP, _PI64]),
    "himut_get_log": (_I, [_P, _P]),
    "himut_get_stats": (_I, [_P, ctypes.POINTER(RunStats)]),
    "himut_set_stage_timing": (_I, [_P, _I]),
    "himut_records_device": (_I, [_P, _PP, _PI64]),
    "himut_copy_records_to_device": (_I, [_P, _P, _I64]),
    "himut_ingest_begin": (_I, [_P, _I64, _I64]),
    "himut_ingest_buffer": (_P, [_P, _I]),
    "himut_ingest_wait": (_I, [_P, _I]),
    "himut_ingest_window": (_I, [_P, _I, _I64, _I64, _P, _P, _I64, _I64, _I64]),
    "himut_ingest_end": (_I, [_P, _I, ctypes.POINTER(IngestResult)]),
    "himut_ingest_derive_cs": (_I, [_P, _I]),
    "himut_ingest_derive_result": (_I, [_P, _P]),
    "himut_ingest_read_meta": (_I, [_P] * 6),
    "himut_download_reads": (_I, [_P, ctypes.POINTER(ReadBatchStruct), _P]),
    "himut_set_reference": (_I, [_P, _P, _I64, _P, _I]),
    "himut_run_normcounts": (_I, [_P, _P, _I]),
    "himut_get_normcounts": (_I, [_P, _P, _P, _P]),
    "himut_debug_normcounts": (_I, [_P, _I, _I64, _I]),
    "himut_debug_norm_scratch": (_I, [_P, _P]),
    "himut_debug_norm_callable": (_I, [_P, _P, _I64, _P, _I64]),
    "himut_ref_tricounts": (_I, [_P, _P]),
    "himut_fasta_tricounts": (_I, [_P, _P, _I64, _P]),
    "himut_debug_fasta_window": (_I, [_P, _I64]),
    "himut_sbs96_counts": (_I, [_P, _P, _P, _P, _I64, _P]),
    "himut_sbs1536_counts": (_I, [_P, _P, _P, _P, _I64, _P]),
    "himut_id83_classify": (_I, [_P, _P, _P, _P, _P, _I64, _P, _P]),
    "himut_dbs78_counts": (_I, [_P, _P, _P, _I64, _P, _P]),
    "himut_debug_spectra": (_I, [_P, _I]),
    "himut_fit_exposures": (_I, [_P, _P, _I32, _I32, _P, _I32, ctypes.c_uint64, _I32, _P, _P]),
    "himut_debug_fit": (_I, [_P, _I, _I]),
    "himut_set_strands": (_I, [_P, _P, _P, _I64]),
    "himut_sbs384_counts": (_I, [_P, _P, _P, _P, _I64, _P, _P]),
    "himut_strand_tricounts": (_I, [_P, _P]),
    "himut_strand_callable": (_I, [_P, _P, _P]),
    "himut_run_edges": (_I, [_P, _P, _P, _I64, _I, _I, _I64, _P]),
    "himut_run_germline": (_I, [_P, ctypes.POINTER(GermlineParams)]),
    "himut_get_germline": (_I, [_P, _PP, _PI64, _P]),
    "himut_run_support": (_I, [_P, _P, _P, _P, _I64, ctypes.POINTER(SupportParams)]),
    "himut_get_support": (_I, [_P, _PP, _PI64, _PP]),
    "himut_run_bqcal": (_I, [_P, ctypes.POINTER(BqcalParams)]),
    "himut_get_bqcal": (_I, [_P, _P, _P, _P]),
    "himut_debug_bqcal": (_I, [_P, _I]),
    "himut_debug_decode": (_I, [_P, _I]),
    "himut_debug_read_pass_sizes": (_I, [_P, _P]),
    "himut_debug_read_pass": (_I, [_P] * 12),
    "himut_run_callable": (_I, [_P, _P, _I]),
    "himut_get_callable": (_I, [_P, _PP, _PI64, _P]),
    "himut_get_callable_map": (_I, [_P, _P, _P, _I64]),
    "himut_run_intervals": (_I, [_P, _P, _P, _I64]),
    "himut_get_intervals": (_I, [_P, _PP, _PI64]),
    "himut_run_dbs": (_I, [_P]),
    "himut_get_dbs": (_I, [_P, _PP, _PI64, _P]),
    "himut_run_sites": (_I, [_P, _P, _P, _P, _I64]),
    "himut_get_sites": (_I, [_P, _PP, _PI64, _P]),
    "himut_run_indels": (_I, [_P, ctypes.POINTER(IndelParams)]),
    "himut_get_indels": (_I, [_P, _PP, _PI64, _P]),
    "himut_run_indelcal": (_I, [_P, ctypes.POINTER(IndelcalParams)]),
    "himut_get_indelcal": (_I, [_P, _P, _P]),
    "himut_set_indel_error_table": (_I, [_P, _P, _P, _I64]),
    "himut_debug_indelcal": (_I, [_P, _I, _I64]),
    "himut_run_sindels": (_I, [_P, ctypes.POINTER(SindelParams)]),
    "himut_get_sindels": (_I, [_P, _PP, _PI64, _P]),
    "himut_run_haplotag": (_I, [_P, _P, _P, _P, _P, _P, _I64, _I32, ctypes.POINTER(HaplotagParams)]),
    "himut_get_haplotag": (_I, [_P, _PP, _PI64, _PP, _PI64, _P]),
    "himut_run_duplex": (_I, [_P, _P, _I64, ctypes.POINTER(DuplexParams)]),
    "himut_get_duplex": (_I, [_P, _PP, _PI64, _P, _P]),
    "himut_get_read_info": (_I, [_P, _P, _P, _P, _P]),
    "himut_pile_counts": (_I, [_P, _I32, _I32, _P, _P]),
}
EXPORTS = list(_ABI)

_lib = None


class HimutError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("libhimut_hip error {}: {}".format(code, message))
        self.code = code
        self.message = message


def _maybe_import_torch_first():
    """torch ships its own libamdhip64.so.7; whichever copy is loaded first
    serves the whole process.  When torch is going to be used in this process
    (bench.py, the RCCL gather) it must come up before our library so both bind
    to the same HIP runtime instance."""
    if "torch" in sys.modules or os.environ.get("HIMUT_NO_TORCH") == "1":
        return
    if os.environ.get("HIMUT_WITH_TORCH") == "1":
        import torch  # noqa: F401


def lib():
    global _lib
    if _lib is not None:
        return _lib
    _maybe_import_torch_first()
    path = os.environ.get("HIMUT_HIP_LIB_OVERRIDE") or build.HIP_LIB   # override: diagnostic builds only
    if not os.path.exists(path):
        path = build.build_hip()
    L = ctypes.CDLL(path)
    for name, (restype, argtypes) in _ABI.items():
        if not hasattr(L, name):
            raise ImportError("libhimut_hip.so lacks symbol " + name)
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    if L.himut_abi_version() != 2:
        raise ImportError("libhimut_hip.so ABI version mismatch")
    _lib = L
    return L


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _copied(address, count, dtype):
    """A host copy of ``count`` items of ``dtype`` that the library holds at ``address``; empty for none."""
    dtype = np.dtype(dtype)
    if not count:
        return np.zeros(0, dtype)
    return np.frombuffer((ctypes.c_char * (count * dtype.itemsize)).from_address(address), dtype=dtype).copy()


def _site_arrays(who, pos1, ref, alt):
    """A site list as the three contiguous arrays a run takes: int32 positions, ASCII ref / alt from arrays of bytes or a
    bytes object each."""
    pos1 = np.ascontiguousarray(pos1, np.int32)
    ref = np.ascontiguousarray(np.frombuffer(ref, np.uint8) if isinstance(ref, (bytes, bytearray)) else ref, np.uint8)
    alt = np.ascontiguousarray(np.frombuffer(alt, np.uint8) if isinstance(alt, (bytes, bytearray)) else alt, np.uint8)
    if not (pos1.shape == ref.shape == alt.shape and pos1.ndim == 1):
        raise ValueError("{}: pos1, ref and alt must be one-dimensional and equally long".format(who))
    return pos1, ref, alt


class Context:
    """One worker bound to one GPU (himut_ctx)."""

    def __init__(self, device=0):
        self._L = lib()
        h = ctypes.c_void_p()
        rc = self._L.himut_create(int(device), ctypes.byref(h))
        if rc:
            raise HimutError(rc, "himut_create failed (no usable HIP device {}?)".format(device))
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._L.himut_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc:
            raise HimutError(rc, self._L.himut_last_error(self._h).decode("utf-8", "replace"))

    def set_params(self, **kw):
        p = Params()
        for k, _ in Params._fields_:
            if k in kw:
                setattr(p, k, kw[k])
        self._check(self._L.himut_set_params(self._h, ctypes.byref(p)))

    def set_gt_lut(self, hom, het, err, log_prior):
        hom = np.ascontiguousarray(hom, np.float64)
        het = np.ascontiguousarray(het, np.float64)
        err = np.ascontiguousarray(err, np.float64)
        pr = np.ascontiguousarray(log_prior, np.float64)
        self._check(self._L.himut_set_gt_lut(self._h, _ptr(hom), _ptr(het), _ptr(err), int(hom.shape[0]), _ptr(pr)))

    def set_chunks(self, chunks):
        s = np.array([c[0] for c in chunks], np.int32)
        e = np.array([c[1] for c in chunks], np.int32)
        self._check(self._L.himut_set_chunks(self._h, _ptr(s), _ptr(e), len(chunks)))

    def set_site_set(self, which, keys):
        k = np.ascontiguousarray(keys, np.uint64)
        self._check(self._L.himut_set_site_set(self._h, int(which), _ptr(k), int(k.shape[0])))

    def set_phase(self, off, hpos, href, halt, hbit):
        off = np.ascontiguousarray(off, np.int64)
        arrs = [np.ascontiguousarray(hpos, np.int32), np.ascontiguousarray(href, np.uint8),
                np.ascontiguousarray(halt, np.uint8), np.ascontiguousarray(hbit, np.uint8)]
        self._check(self._L.himut_set_phase(self._h, _ptr(off), *[_ptr(a) for a in arrs], int(off.shape[0]) - 1))

    def push_reads(self, b):
        keep = {k: np.ascontiguousarray(getattr(b, k), dt) for k, dt in READ_ARRAYS}
        st = ReadBatchStruct.of(b.n, keep)
        self._check(self._L.himut_push_reads(self._h, ctypes.byref(st)))

    def run(self):
        self._check(self._L.himut_run(self._h))

    def _records_and_log(self, getter, dtype, n_log):
        """(records, counters) through a getter of the form (ctx, &pointer, &count, log[n_log])."""
        p = ctypes.c_void_p()
        n = ctypes.c_int64()
        log = np.zeros(n_log, np.int64)
        self._check(getter(self._h, ctypes.byref(p), ctypes.byref(n), _ptr(log)))
        return _copied(p.value, n.value, dtype), [int(x) for x in log]

    def run_begin(self):
        """The run queued, not waited for (run_end does that): several contexts' runs back to back on one GPU."""
        self._check(self._L.himut_run_begin(self._h))

    def run_end(self):
        self._check(self._L.himut_run_end(self._h))

    def run_germline(self, min_mapq=0, min_gq=20, min_bq=20, min_ref_count=2, min_alt_count=2, md_threshold=1 << 30,
                     report_homref=False):
        """The germline run (himut_run_germline) over the context's tables, regions and reads."""
        p = GermlineParams(int(min_mapq), int(min_gq), int(min_bq), int(min_ref_count), int(min_alt_count),
                           int(md_threshold), 1 if report_homref else 0, 0)
        self._check(self._L.himut_run_germline(self._h, ctypes.byref(p)))

    def germline(self):
        """(records, the twelve counters) of the last germline run."""
        return self._records_and_log(self._L.himut_get_germline, RECORD_DTYPE, 12)

    def debug_decode(self, mode):
        """Test hook (himut_debug_decode): 0 = the decode groups consecutive reads (the default), 1 = every read on its own;
        from here on the decode counts its groups and keeps its position bitmap for read_pass()."""
        self._check(self._L.himut_debug_decode(self._h, int(mode)))

    def read_pass(self):
        """Test hook (himut_debug_read_pass): what the last read pass left, as a dict -- nseg, nmis, nnsub, rflag, meta
        (READ_META_DTYPE) per read; segs (SEG_DTYPE), mis, mq per slot; bits (the position bitmap, empty when the pass
        set none); counters (groups, multi-read groups, reads planned per read, reads redone); plan_ms."""
        sz = np.zeros(3, np.int64)
        self._check(self._L.himut_debug_read_pass_sizes(self._h, _ptr(sz)))
        n, slots, words = (int(x) for x in sz)
        out = {"nseg": np.zeros(n, np.int32), "nmis": np.zeros(n, np.int32), "nnsub": np.zeros(n, np.int32),
               "rflag": np.zeros(n, np.uint8), "meta": np.zeros(n, READ_META_DTYPE), "segs": np.zeros(slots, SEG_DTYPE),
               "mis": np.zeros(slots, np.int32), "mq": np.zeros(slots, np.uint32), "bits": np.zeros(words, np.uint32)}
        counters = np.zeros(4, np.int64)
        ms = ctypes.c_double()
        self._check(self._L.himut_debug_read_pass(self._h, *[_ptr(out[k]) for k in ("nseg", "nmis", "nnsub", "rflag", "meta", "segs",
                                                                                      "mis", "mq", "bits")],
                                                  _ptr(counters), ctypes.byref(ms)))
        out["counters"] = [int(x) for x in counters]
        out["plan_ms"] = float(ms.value)
        return out

    def run_support(self, pos1, ref, alt, min_mapq=0, mismatch_window_size=20):
        """The support run (himut_run_support) over the context's reads: sites (1-based pos non-decreasing, ASCII ref /
        alt as arrays of bytes or a bytes object each)."""
        pos1, ref, alt = _site_arrays("run_support", pos1, ref, alt)
        p = SupportParams(int(min_mapq), int(mismatch_window_size))
        self._check(self._L.himut_run_support(self._h, _ptr(pos1), _ptr(ref), _ptr(alt), int(pos1.shape[0]), ctypes.byref(p)))
        self._n_support_sites = int(pos1.shape[0])

    def support(self):
        """(rows as SUPPORT_ROW_DTYPE ascending by (site, read), site_counts[n_sites, 2] = cover, alt_reads) of the last
        support run."""
        p = ctypes.c_void_p()
        q = ctypes.c_void_p()
        n = ctypes.c_int64()
        self._check(self._L.himut_get_support(self._h, ctypes.byref(p), ctypes.byref(n), ctypes.byref(q)))
        ns = getattr(self, "_n_support_sites", 0)
        return _copied(p.value, n.value, SUPPORT_ROW_DTYPE), _copied(q.value, ns * 2, np.int32).reshape(ns, 2)

    def run_haplotag(self, pos1, ref, alt, bit, set, n_sets=None, min_mapq=0, min_bq=20, min_snps=1, min_agree_permille=800):
        """The haplotag run (himut_run_haplotag) over the context's reads: the contig's phased hetSNPs as parallel arrays
        (1-based pos strictly ascending, ASCII ref / alt as arrays of bytes or a bytes object each, bit = the allele on
        the first haplotype, set = the phase set's index below ``n_sets``; None: the largest index + 1)."""
        pos1, ref, alt = _site_arrays("run_haplotag", pos1, ref, alt)
        bit, set = np.ascontiguousarray(bit, np.uint8), np.ascontiguousarray(set, np.int32)
        if not (bit.shape == set.shape == pos1.shape):
            raise ValueError("run_haplotag: bit and set must be as long as pos1")
        if n_sets is None:
            n_sets = int(set.max(initial=-1)) + 1
        p = HaplotagParams(int(min_mapq), int(min_bq), int(min_snps), int(min_agree_permille))
        self._check(self._L.himut_run_haplotag(self._h, _ptr(pos1), _ptr(ref), _ptr(alt), _ptr(bit), _ptr(set),
                                               int(pos1.shape[0]), int(n_sets), ctypes.byref(p)))

    def haplotag(self):
        """(rows as HAPLOTAG_ROW_DTYPE, one per read; snps as HAPLOTAG_SNP_DTYPE, one per hetSNP; the thirteen counters)
        of the last haplotag run."""
        p, q = ctypes.c_void_p(), ctypes.c_void_p()
        n, m = ctypes.c_int64(), ctypes.c_int64()
        log = np.zeros(13, np.int64)
        self._check(self._L.himut_get_haplotag(self._h, ctypes.byref(p), ctypes.byref(n), ctypes.byref(q), ctypes.byref(m), _ptr(log)))
        return _copied(p.value, n.value, HAPLOTAG_ROW_DTYPE), _copied(q.value, m.value, HAPLOTAG_SNP_DTYPE), [int(x) for x in log]

    def run_duplex(self, mate):
        """The duplex run (himut_run_duplex) over the context's parameters, tables, regions, site sets and reads:
        ``mate[i]`` the read on the other strand of read i's molecule, or -1 (duplex.mate_index)."""
        mate = np.ascontiguousarray(mate, np.int32)
        if mate.ndim != 1:
            raise ValueError("run_duplex: mate must be one-dimensional")
        p = DuplexParams()
        self._check(self._L.himut_run_duplex(self._h, _ptr(mate) if mate.shape[0] else None, int(mate.shape[0]), ctypes.byref(p)))

    def duplex(self):
        """(records as DUPLEX_RECORD_DTYPE ascending by (tpos, ref, alt), ss[12] in the order of DUPLEX_SS_CLASSES, the
        forty counters of DUPLEX_LOG_NAMES) of the last duplex run."""
        p = ctypes.c_void_p()
        n = ctypes.c_int64()
        ss, log = np.zeros(12, np.int64), np.zeros(40, np.int64)
        self._check(self._L.himut_get_duplex(self._h, ctypes.byref(p), ctypes.byref(n), _ptr(ss), _ptr(log)))
        return _copied(p.value, n.value, DUPLEX_RECORD_DTYPE), [int(x) for x in ss], [int(x) for x in log]

    def read_info(self, n):
        """(tstart, tend, flag, mapq) of the context's ``n`` reads, pushed or ingested (himut_get_read_info): what a table
        with a line per read says beside a run's row."""
        a = [np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint16), np.zeros(n, np.uint8)]
        self._check(self._L.himut_get_read_info(self._h, *[_ptr(x) for x in a]))
        return a

    def run_bqcal(self, min_mapq=0, min_gq=20, md_threshold=1 << 30):
        """The bqcal run (himut_run_bqcal) over the context's tables, regions (0-based, half open), reference string
        and reads."""
        p = BqcalParams(int(min_mapq), int(min_gq), int(md_threshold))
        self._check(self._L.himut_run_bqcal(self._h, ctypes.byref(p)))

    def bqcal(self):
        """(match[256], mismatch[256] indexed by BQ, the twelve counters) of the last bqcal run."""
        match, mismatch, log = np.zeros(256, np.int64), np.zeros(256, np.int64), np.zeros(12, np.int64)
        self._check(self._L.himut_get_bqcal(self._h, _ptr(match), _ptr(mismatch), _ptr(log)))
        return match, mismatch, [int(x) for x in log]

    def debug_bqcal(self, row_batch=0):
        """Test hook (himut_debug_bqcal): pile rows of a tile held in LDS at a time, 0 = the default."""
        self._check(self._L.himut_debug_bqcal(self._h, int(row_batch)))

    def run_dbs(self):
        """The dbs run (himut_run_dbs) over the context's parameters, tables, regions, site sets and reads."""
        self._check(self._L.himut_run_dbs(self._h))

    def dbs(self):
        """(records as DBS_RECORD_DTYPE ascending by (tpos, alt1, alt2), the twenty counters) of the last dbs run."""
        return self._records_and_log(self._L.himut_get_dbs, DBS_RECORD_DTYPE, 20)

    def run_sites(self, pos1, ref, alt):
        """The sites run (himut_run_sites) over the context's parameters, tables, site sets and reads: sites (1-based pos
        non-decreasing, ASCII ref / alt as arrays of bytes or a bytes object each)."""
        pos1, ref, alt = _site_arrays("run_sites", pos1, ref, alt)
        self._check(self._L.himut_run_sites(self._h, _ptr(pos1), _ptr(ref), _ptr(alt), int(pos1.shape[0])))

    def sites(self):
        """(records as SITE_RECORD_DTYPE in input order, the twenty counters) of the last sites run."""
        return self._records_and_log(self._L.himut_get_sites, SITE_RECORD_DTYPE, 20)

    def run_indels(self, min_mapq=0, min_gq=20, min_ref_count=2, min_alt_count=2, md_threshold=1 << 30, max_len=50,
                   indel_error=0.01, germline_indel_prior=1 / (10 ** 4), report_homref=False):
        """The indels run (himut_run_indels) over the context's regions, reference string and reads."""
        lg = indel_logs(indel_error, germline_indel_prior)
        p = IndelParams(int(min_mapq), int(min_gq), int(min_ref_count), int(min_alt_count), int(md_threshold), int(max_len),
                        1 if report_homref else 0, 0, lg[0], lg[1], lg[2], (ctypes.c_double * 3)(*lg[3:]))
        self._check(self._L.himut_run_indels(self._h, ctypes.byref(p)))

    def indels(self):
        """(records as INDEL_RECORD_DTYPE ascending by (anchor, type, length, inserted bases), the thirteen counters) of
        the last indels run."""
        return self._records_and_log(self._L.himut_get_indels, INDEL_RECORD_DTYPE, 13)

    def run_sindels(self, min_mapq=20, min_gq=20, min_ref_count=3, min_alt_count=1, md_threshold=1 << 30, max_len=50,
                    max_run=2, min_qv=30, indel_error=0.01, germline_indel_prior=1 / (10 ** 4), qlen_lower_limit=-1,
                    qlen_upper_limit=(1 << 31) - 1, min_bq=93, mismatch_window_size=20, max_mismatch_count=0,
                    min_sequence_identity=0.99, min_trim=0.01):
        """The sindels run (himut_run_sindels) over the context's regions, reference string, reads and, where one is
        set, indel error table."""
        lg = indel_logs(indel_error, germline_indel_prior)
        p = SindelParams(int(min_mapq), int(min_gq), int(min_ref_count), int(min_alt_count), int(md_threshold), int(max_len),
                         int(max_run), int(min_qv), lg[0], lg[1], lg[2], (ctypes.c_double * 3)(*lg[3:]),
                         int(qlen_lower_limit), int(qlen_upper_limit), int(min_bq), int(mismatch_window_size),
                         int(max_mismatch_count), 0, float(min_sequence_identity), float(min_trim))
        self._check(self._L.himut_run_sindels(self._h, ctypes.byref(p)))

    def sindels(self):
        """(records as SINDEL_RECORD_DTYPE ascending by (anchor, type, length, inserted bases), the twenty counters of
        SINDEL_LOG_NAMES) of the last sindels run."""
        return self._records_and_log(self._L.himut_get_sindels, SINDEL_RECORD_DTYPE, 20)

    def run_indelcal(self, min_mapq=0, max_len=50, min_alt_count=2, vaf_permille=250):
        """The indelcal run (himut_run_indelcal) over the context's regions, reference string and reads."""
        p = IndelcalParams(int(min_mapq), int(max_len), int(min_alt_count), int(vaf_permille))
        self._check(self._L.himut_run_indelcal(self._h, ctypes.byref(p)))

    def indelcal(self):
        """(table[128, 10] in the columns of INDELCAL_COLUMNS, the fourteen counters) of the last indelcal run."""
        table, log = np.zeros((INDELCAL_CLASSES, len(INDELCAL_COLUMNS)), np.int64), np.zeros(14, np.int64)
        self._check(self._L.himut_get_indelcal(self._h, _ptr(table), _ptr(log)))
        return table, [int(x) for x in log]

    def debug_indelcal(self, sweep_workgroups=0, cell_budget=0):
        """Test hook (himut_debug_indelcal): workgroups of the span sweep and the budget of its histogram cells, 0 = the default."""
        self._check(self._L.himut_debug_indelcal(self._h, int(sweep_workgroups), int(cell_budget)))

    def set_indel_error_table(self, l_hit=None, l_err=None):
        """The per-read terms the indels runs that follow take per (run class, event column) cell
        (himut_set_indel_error_table): two arrays of INDEL_ERROR_CELLS doubles, log10(1 - e) and log10(e); without
        arguments the table is cleared and the runs use their constant again."""
        if l_hit is None and l_err is None:
            self._check(self._L.himut_set_indel_error_table(self._h, None, None, 0))
            return
        l_hit, l_err = np.ascontiguousarray(l_hit, np.float64), np.ascontiguousarray(l_err, np.float64)
        if l_hit.shape != l_err.shape or l_hit.ndim != 1:
            raise ValueError("set_indel_error_table: l_hit and l_err must be one-dimensional and equally long")
        self._check(self._L.himut_set_indel_error_table(self._h, _ptr(l_hit), _ptr(l_err), int(l_hit.shape[0])))

    def records(self):
        p = ctypes.c_void_p()
        n = ctypes.c_int64()
        self._check(self._L.himut_get_records(self._h, ctypes.byref(p), ctypes.byref(n)))
        return _copied(p.value, n.value, RECORD_DTYPE)

    def log(self):
        out = np.zeros(15, np.int64)
        self._check(self._L.himut_get_log(self._h, _ptr(out)))
        return [int(x) for x in out]

    def stats(self):
        s = RunStats()
        self._check(self._L.himut_get_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def stats_brief(self):
        """(ms_total, ms_capture, reran) of the last run without building the whole dictionary: what a timed loop reads."""
        s = getattr(self, "_st", None)
        if s is None:
            s = self._st = RunStats()
        self._L.himut_get_stats(self._h, ctypes.byref(s))
        return s.ms_total, s.ms_capture, s.reran

    def set_stage_timing(self, level):
        """0: total only; 1: + column capture (default); 2: every stage (costs a few microseconds per event)."""
        self._check(self._L.himut_set_stage_timing(self._h, int(level)))

    def records_device(self):
        p = ctypes.c_void_p()
        n = ctypes.c_int64()
        self._check(self._L.himut_records_device(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def copy_records_to_device(self, dev_ptr, capacity_records):
        self._check(self._L.himut_copy_records_to_device(self._h, ctypes.c_void_p(dev_ptr), int(capacity_records)))

    def set_reference(self, seq, cls, n_classes):
        raw = np.frombuffer(seq.encode("ascii") if isinstance(seq, str) else bytes(seq), np.uint8)
        cls = np.ascontiguousarray(cls, np.uint8)
        self._n_classes = int(n_classes)
        self._check(self._L.himut_set_reference(self._h, _ptr(raw), int(raw.shape[0]), _ptr(cls), int(n_classes)))

    def run_normcounts(self, alt_order, non_human_sample=False):
        tab = np.ascontiguousarray(alt_order, np.uint8).reshape(12)
        self._check(self._L.himut_run_normcounts(self._h, _ptr(tab), 1 if non_human_sample else 0))

    def debug_normcounts(self, sweep=0, dirty_cap=0, pool_slots=0):
        """Test hook (himut_debug_normcounts): which sweep (0 k_norm_quad, 1 k_norm_tile, 2 as 0 with the first pass taken as
        if its list of tiles had been too short: the whole-contig repeat), the capacity of a part of the left-over list,
        pool slots."""
        self._check(self._L.himut_debug_normcounts(self._h, int(sweep), int(dirty_cap), int(pool_slots)))

    def norm_scratch(self):
        """Test hook (himut_debug_norm_scratch): device bytes held for the normcounts sweep -- plan, left-over position
        list, tile list, total."""
        out = (ctypes.c_int64 * 4)()
        self._check(self._L.himut_debug_norm_scratch(self._h, out))
        return [int(v) for v in out]

    def norm_callable(self, n_words, n_reads):
        """Test hook (himut_debug_norm_callable): (words, live) of the last completed normcounts pass -- bit q & 31 of
        word (qoff[r] + q) >> 5 is query base q of read r; live[r]: the read passed the read filters."""
        words, live = np.zeros(int(n_words), np.uint32), np.zeros(int(n_reads), np.uint8)
        self._check(self._L.himut_debug_norm_callable(self._h, _ptr(words), int(n_words), _ptr(live), int(n_reads)))
        return words, live

    def normcounts(self):
        k3 = self._n_classes ** 3
        ccs = np.zeros(k3, np.int64)
        ref = np.zeros(k3, np.int64)
        log = np.zeros(14, np.int64)
        self._check(self._L.himut_get_normcounts(self._h, _ptr(ccs), _ptr(ref), _ptr(log)))
        return ccs, ref, [int(x) for x in log]

    def run_callable(self, alt_order, non_human_sample=False):
        """The callable run (himut_run_callable): the inputs of run_normcounts, a state and the callable bases per swept
        position, and the runs of equal state."""
        tab = np.ascontiguousarray(alt_order, np.uint8).reshape(12)
        self._check(self._L.himut_run_callable(self._h, _ptr(tab), 1 if non_human_sample else 0))

    def callable(self):
        """(runs as CALLABLE_RUN_DTYPE in chunk order, ascending within a chunk; the fourteen counters of norm.log) of
        the last callable run."""
        return self._records_and_log(self._L.himut_get_callable, CALLABLE_RUN_DTYPE, 14)

    def callable_map(self, n):
        """(state[n] as uint8, bases[n] as uint16): the first ``n`` entries of the last callable run's per-position map,
        the chunks' positions one behind the other in chunk order."""
        state, bases = np.zeros(int(n), np.uint8), np.zeros(int(n), np.uint16)
        self._check(self._L.himut_get_callable_map(self._h, _ptr(state), _ptr(bases), int(n)))
        return state, bases

    def run_intervals(self, start, end):
        """The intervals run (himut_run_intervals): the last completed callable run's map tallied inside each interval
        (start[i], end[i]), 0-based and half open, any order."""
        start, end = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(end, np.int32)
        if not (start.shape == end.shape and start.ndim == 1):
            raise ValueError("run_intervals: start and end must be one-dimensional and equally long")
        self._check(self._L.himut_run_intervals(self._h, _ptr(start), _ptr(end), int(start.shape[0])))

    def intervals(self):
        """The rows (INTERVAL_ROW_DTYPE, input order) of the last intervals run."""
        p = ctypes.c_void_p()
        n = ctypes.c_int64()
        self._check(self._L.himut_get_intervals(self._h, ctypes.byref(p), ctypes.byref(n)))
        return _copied(p.value, n.value, INTERVAL_ROW_DTYPE)

    def run_edges(self, hpos, href, min_bq, min_mapq, band):
        hpos = np.ascontiguousarray(hpos, np.int32)
        href = np.ascontiguousarray(href, np.uint8)
        counts = np.zeros(max(1, hpos.shape[0]) * int(band) * 4, np.uint32)
        self._check(self._L.himut_run_edges(self._h, _ptr(hpos), _ptr(href), int(hpos.shape[0]), int(min_bq), int(min_mapq),
                                            int(band), _ptr(counts)))
        return counts

    def ref_tricounts(self):
        out = np.zeros(64, np.int64)
        self._check(self._L.himut_ref_tricounts(self._h, _ptr(out)))
        return out

    # ---- device-side BAM ingest (bamio.ingest_contig drives it)
    def ingest_begin(self, inflated_bound, window_bytes):
        self._check(self._L.himut_ingest_begin(self._h, int(inflated_bound), int(window_bytes)))
        return [self._L.himut_ingest_buffer(self._h, k) for k in (0, 1)]

    @property
    def handle(self):
        """The himut_ctx* (for a host library that calls the C ABI itself: bamio's ingest pump)."""
        return self._h

    def fn_address(self, name):
        """Address of an exported function of the library, as a void*."""
        return ctypes.cast(getattr(self._L, name), ctypes.c_void_p)

    def raise_for(self, rc):
        self._check(rc)

    def ingest_wait(self, slot):
        self._check(self._L.himut_ingest_wait(self._h, int(slot)))

    def ingest_window(self, slot, start, nbytes, rec_off, qid, n_rec, padded_bases, tag_bytes):
        self._check(self._L.himut_ingest_window(self._h, int(slot), int(start), int(nbytes), _ptr(rec_off), _ptr(qid),
                                                int(n_rec), int(padded_bases), int(tag_bytes)))

    def ingest_end(self, unique_qnames):
        r = IngestResult()
        rc = self._L.himut_ingest_end(self._h, 1 if unique_qnames else 0, ctypes.byref(r))
        self._check(rc)
        return {k: getattr(r, k) for k, _ in IngestResult._fields_}

    def ingest_derive_cs(self, mode):
        """0: the cs tags of the records are the text (default).  1: the ingests that follow derive the text of every
        record from CIGAR, SEQ and the string given to set_reference."""
        self._check(self._L.himut_ingest_derive_cs(self._h, int(mode)))

    def ingest_derive_result(self):
        """Of the last ingest: records derived, underivable records, bytes of derived text, device ms of the post-pass."""
        out = (ctypes.c_int64 * 4)()
        self._check(self._L.himut_ingest_derive_result(self._h, out))
        return dict(zip(("n_derived", "n_underivable", "cs_bytes", "ms"), (int(v) for v in out)))

    def ingest_read_meta(self, n):
        """(tstart, tend, qlen, mapq, tp) of the resident reads: what bamlib.get_thresholds looks at."""
        a = [np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)]
        self._check(self._L.himut_ingest_read_meta(self._h, *[_ptr(x) for x in a]))
        return a

    def download_reads(self, res, name="", length=0):
        """The resident read batch as a host ReadBatch (tests)."""
        n = int(res["n_reads"])
        a = read_arrays(n, seq=int(res["bases_padded"]) // 2, bq=int(res["bases_padded"]), cs=int(res["cs_bytes"]))
        tp = np.zeros(n, np.uint8)
        st = ReadBatchStruct.of(n, a)
        self._check(self._L.himut_download_reads(self._h, ctypes.byref(st), _ptr(tp)))
        return ReadBatch(name=name, length=length, tp=tp, **a)

    def sbs96_counts(self, pos0, ref, alt):
        """99 bins (see himut_sbs96_counts) for the substitutions (0-based pos, ASCII ref / alt) of the contig whose
        string was given to set_reference."""
        return self._sbs_counts(self._L.himut_sbs96_counts, 99, pos0, ref, alt)

    def sbs1536_counts(self, pos0, ref, alt):
        """1539 bins (see himut_sbs1536_counts), as sbs96_counts."""
        return self._sbs_counts(self._L.himut_sbs1536_counts, 1539, pos0, ref, alt)

    def _sbs_counts(self, fn, nbins, pos0, ref, alt):
        pos0 = np.ascontiguousarray(pos0, np.int32)
        ref = np.ascontiguousarray(ref, np.uint8)
        alt = np.ascontiguousarray(alt, np.uint8)
        out = np.zeros(nbins, np.int64)
        self._check(fn(self._h, _ptr(pos0), _ptr(ref), _ptr(alt), int(pos0.shape[0]), _ptr(out)))
        return out

    def id83_classify(self, anchor0, type, len, bases=None, want_classes=True):
        """(cls, 88 bins) (see himut_id83_classify) for indel alleles of the contig whose string was given to
        set_reference: 0-based anchors, types (0 deletion, 1 insertion), lengths, and the inserted bases as rows of 16
        bytes in the indel record's packing (None: all zero, for a list of deletions).  ``cls`` is None without
        ``want_classes``."""
        anchor0 = np.ascontiguousarray(anchor0, np.int32)
        type = np.ascontiguousarray(type, np.uint8)
        len = np.ascontiguousarray(len, np.int32)
        n = int(anchor0.shape[0])
        bases = np.zeros((n, 16), np.uint8) if bases is None else np.ascontiguousarray(bases, np.uint8).reshape(n, 16)
        if not (anchor0.ndim == 1 and type.shape == len.shape == anchor0.shape):
            raise ValueError("id83_classify: anchor0, type and len must be one-dimensional and equally long")
        cls = np.zeros(n, np.uint8) if want_classes else None
        out = np.zeros(88, np.int64)
        self._check(self._L.himut_id83_classify(self._h, _ptr(anchor0), _ptr(type), _ptr(len), _ptr(bases), n,
                                                _ptr(cls) if want_classes else None, _ptr(out)))
        return cls, out

    def dbs78_counts(self, ref2, alt2, want_classes=True):
        """(cls, 80 bins) (see himut_dbs78_counts) for doublets given as two (n, 2) arrays of ASCII letters."""
        ref2 = np.ascontiguousarray(ref2, np.uint8).reshape(-1, 2)
        alt2 = np.ascontiguousarray(alt2, np.uint8).reshape(-1, 2)
        if ref2.shape != alt2.shape:
            raise ValueError("dbs78_counts: ref2 and alt2 must be equally long")
        n = int(ref2.shape[0])
        cls = np.zeros(n, np.uint8) if want_classes else None
        out = np.zeros(80, np.int64)
        self._check(self._L.himut_dbs78_counts(self._h, _ptr(ref2), _ptr(alt2), n, _ptr(cls) if want_classes else None, _ptr(out)))
        return cls, out

    def debug_spectra(self, max_workgroups=0):
        """Test hook (himut_debug_spectra): the most workgroups of k_id83, k_dbs78 and the strand kernels, 0 = the
        default."""
        self._check(self._L.himut_debug_spectra(self._h, int(max_workgroups)))

    def fit_exposures(self, sig, counts, n_boot=0, seed=1, iters=1000, want_resampled=True):
        """(exposures[n_boot + 1, K], resampled[n_boot + 1, C] as int32) (see himut_fit_exposures) of the counts under the
        signature matrix ``sig`` ([C, K], columns summing to 1): row 0 the counts themselves, rows 1..n_boot the bootstrap
        replicates.  ``resampled`` is None without ``want_resampled``."""
        sig = np.ascontiguousarray(sig, np.float64)
        counts = np.ascontiguousarray(counts, np.int64)
        if sig.ndim != 2 or counts.ndim != 1 or counts.shape[0] != sig.shape[0]:
            raise ValueError("fit_exposures: sig must be [C, K] and counts [C]")
        C, K = (int(x) for x in sig.shape)
        rows = max(int(n_boot), 0) + 1
        expo = np.zeros((rows, K), np.float64)
        res = np.zeros((rows, C), np.int32) if want_resampled else None
        self._check(self._L.himut_fit_exposures(self._h, _ptr(sig), C, K, _ptr(counts), int(n_boot), int(seed) & (2 ** 64 - 1),
                                                int(iters), _ptr(expo), _ptr(res) if want_resampled else None))
        return expo, res

    def debug_fit(self, max_workgroups=0, lds_budget_bytes=0):
        """Test hook (himut_debug_fit): the most workgroups of the fit's kernels and the LDS budget of a workgroup of
        k_fit_em in bytes, 0 = the default."""
        self._check(self._L.himut_debug_fit(self._h, int(max_workgroups), int(lds_budget_bytes)))

    def set_strands(self, seg_start, seg_mask):
        """The transcription-strand segment list (see himut_set_strands) of the contig whose string was given to
        set_reference: ascending starts from 0 and a mask 0..3 per segment."""
        seg_start = np.ascontiguousarray(seg_start, np.int32)
        seg_mask = np.ascontiguousarray(seg_mask, np.uint8)
        if not (seg_start.ndim == 1 and seg_start.shape == seg_mask.shape):
            raise ValueError("set_strands: seg_start and seg_mask must be one-dimensional and equally long")
        self._check(self._L.himut_set_strands(self._h, _ptr(seg_start), _ptr(seg_mask), int(seg_start.shape[0])))

    def sbs384_counts(self, pos0, ref, alt, want_classes=True):
        """(cls, 387 bins) (see himut_sbs384_counts) for the substitutions of sbs96_counts; ``cls`` (uint16, 0xFFFF for a
        flagged substitution) is None without ``want_classes``."""
        pos0 = np.ascontiguousarray(pos0, np.int32)
        ref = np.ascontiguousarray(ref, np.uint8)
        alt = np.ascontiguousarray(alt, np.uint8)
        if not (pos0.ndim == 1 and pos0.shape == ref.shape == alt.shape):
            raise ValueError("sbs384_counts: pos0, ref and alt must be one-dimensional and equally long")
        n = int(pos0.shape[0])
        cls = np.zeros(n, np.uint16) if want_classes else None
        out = np.zeros(387, np.int64)
        self._check(self._L.himut_sbs384_counts(self._h, _ptr(pos0), _ptr(ref), _ptr(alt), n,
                                                _ptr(cls) if want_classes else None, _ptr(out)))
        return cls, out

    def strand_tricounts(self):
        """int64[4, 32] (see himut_strand_tricounts): category x trinucleotide class over the resident string."""
        out = np.zeros(128, np.int64)
        self._check(self._L.himut_strand_tricounts(self._h, _ptr(out)))
        return out.reshape(4, 32)

    def strand_callable(self):
        """(positions, bases), int64[4, 32] each (see himut_strand_callable): the CALLABLE entries of the last callable
        run's map by category and trinucleotide class."""
        pos, bases = np.zeros(128, np.int64), np.zeros(128, np.int64)
        self._check(self._L.himut_strand_callable(self._h, _ptr(pos), _ptr(bases)))
        return pos.reshape(4, 32), bases.reshape(4, 32)

    def fasta_tricounts(self, body):
        """64 bins (see himut_fasta_tricounts) of one record's sequence lines: any object with the buffer protocol
        (bytes, a memoryview of an mmap)."""
        mv = memoryview(body).cast("B")
        out = np.zeros(64, np.int64)
        n = mv.nbytes
        buf = np.frombuffer(mv, np.uint8) if n else np.zeros(1, np.uint8)
        self._check(self._L.himut_fasta_tricounts(self._h, _ptr(buf), n, _ptr(out)))
        return out

    def debug_fasta_window(self, window_bytes=0):
        """Test hook (himut_debug_fasta_window): the staging window in bytes, 0 = the default."""
        self._check(self._L.himut_debug_fasta_window(self._h, int(window_bytes)))

    def pile_counts(self, p0, p1):
        counts = np.zeros((p1 - p0, 6), np.uint32)
        bqsum = np.zeros((p1 - p0, 4), np.uint32)
        self._check(self._L.himut_pile_counts(self._h, int(p0), int(p1), _ptr(counts), _ptr(bqsum)))
        return counts, bqsum
