"""`himut haplotag`: each read's haplotype from a phased VCF.

`himut phase` writes phase sets; `call --phase` and `normcounts --phase` read them through a rule that answers one
all-or-nothing byte per (chunk, read) and keeps it on the device.  This command answers per molecule, over the whole
contig: which phase set and haplotype a read's bases at the phased hetSNPs vote for, how sure that is, and -- per hetSNP
-- what the reads show there and how many assigned reads contradict its phase (switch errors, bad sites).  The reference's
authors assigned molecules with a script outside the package (scripts/sbs2hap.py).  The decoded reads are resident in HBM
already; one kernel turns the hetSNP list into one row per read and one per hetSNP.  The contract -- pile reads, the
classification at a hetSNP, the chosen set, the verdict, the tallies, the counters -- is DESIGN.md section 8 and
include/himut_hip.h (himut_run_haplotag).  There is no CPU implementation: without the HIP library the call raises.
"""
import numpy as np

from .caller import reads_for

READ_COLUMNS = ("chrom", "qname", "start", "end", "strand", "mapq", "PS", "HP", "status", "n_h1", "n_h2", "n_other", "n_del",
                "n_lowbq", "n_sets")
SNP_COLUMNS = ("chrom", "pos", "ref", "alt", "gt", "PS", "depth", "n_ref", "n_alt", "n_other", "n_del", "n_lowbq", "agree",
               "disagree")
# himut_haplotag.log: the run's thirteen counters, then what the host derives from the hetSNP rows
LOG_ROWS = ("num_reads", "num_pile_reads", "num_hap1_reads", "num_hap2_reads", "num_no_snp_reads", "num_no_vote_reads",
            "num_low_support_reads", "num_conflict_reads", "num_multi_set_reads", "num_votes", "num_other_bases",
            "num_deleted_bases", "num_low_bq_bases", "num_phased_hetsnps", "num_spanned_hetsnps", "num_disagreeing_hetsnps")


def agree_permille(min_agree):
    """--min_agree as the integer the device compares with: max(n0, n1) * 1000 >= permille * (n0 + n1)."""
    v = int(round(float(min_agree) * 1000))
    if not 501 <= v <= 1000:
        raise ValueError("min_agree must lie in 0.501 .. 1")
    return v


class PhasedSnps:
    """The phased hetSNPs of one contig as the five parallel arrays of the run, by position; names[k]: the VCF's PS string
    of set k (the sets are numbered by their first position); duplicates: positions listed twice (the first is kept)."""

    def __init__(self, pos1, ref, alt, bit, set, names, duplicates=0):
        self.pos1, self.ref, self.alt = np.asarray(pos1, np.int32), np.asarray(ref, np.uint8), np.asarray(alt, np.uint8)
        self.bit, self.set = np.asarray(bit, np.uint8), np.asarray(set, np.int32)
        self.names, self.duplicates = list(names), int(duplicates)

    def __len__(self):
        return int(self.pos1.shape[0])

    def tuples(self):
        """[(pos1, ref, alt, bit, set)] with the letters as str."""
        return [(int(p), chr(r), chr(a), int(b), int(s)) for p, r, a, b, s in zip(self.pos1, self.ref, self.alt, self.bit, self.set)]


def flatten_sets(ps2hbit, ps2hetsnp, order):
    """PhasedSnps of one contig from vcflib.load_phased_hetsnps' dicts of that contig (PS -> first GT fields, PS ->
    (pos, ref, alt)) and vcflib.phased_record_order's of it ((pos, PS) -> the record's line in the file): those dicts are
    keyed by set, so only the line numbers say which of two records of different sets is the file's first.  A record
    whose alleles are not two different single letters of ACGT cannot vote and is left out."""
    by_first = sorted((hs[0][0], k) for k, (ps, hs) in enumerate(ps2hetsnp.items()) if hs)
    keys = list(ps2hetsnp)
    index = {keys[k]: i for i, (_first, k) in enumerate(by_first)}
    flat = []
    for ps, hs in ps2hetsnp.items():
        for (pos, ref, alt), g in zip(hs, ps2hbit[ps]):
            if len(ref) == 1 and len(alt) == 1 and ref in "ACGT" and alt in "ACGT" and ref != alt:
                flat.append((int(pos), order[(int(pos), ps)], ref, alt, 1 if g == "1" else 0, index[ps]))
    # by position, then by line; stable, so a position one set lists twice keeps that set's own (file) order
    flat.sort(key=lambda s: s[:2])
    kept, dup = [], 0
    for s in flat:
        if kept and kept[-1][0] == s[0]:
            dup += 1
        else:
            kept.append(s)
    names = [str(keys[k]) for _first, k in by_first]
    return PhasedSnps([s[0] for s in kept], [ord(s[2]) for s in kept], [ord(s[3]) for s in kept], [s[4] for s in kept],
                      [s[5] for s in kept], names, dup)


def load_phased(vcf_file, chrom_lst, tname2tsize):
    """(contig -> PhasedSnps for the contigs of ``chrom_lst`` the phased VCF, plain .vcf or .bgz, has 0|1 / 1|0 records
    of; contig -> the number of such records, for the contigs of the file that ``tname2tsize`` -- the BAM -- lacks).  The
    sets come from vcflib.load_phased_hetsnps, the reading `call --phase` has of the file; one more pass over it
    (vcflib.phased_record_order) gives the records' order and the file's contigs.  Of a position listed twice the
    record that stands first in the file is kept; prints how many were dropped."""
    from . import vcflib
    order = vcflib.phased_record_order(vcf_file)
    absent = {c: len(v) for c, v in order.items() if c not in tname2tsize}
    sizes = dict(tname2tsize)
    sizes.update(dict.fromkeys(absent, 0))              # (load_phased_hetsnps files a plain .vcf's records under every contig it meets)
    hbit, _hpos, hsnp, _chunks = vcflib.load_phased_hetsnps(vcf_file, list(chrom_lst), sizes)
    out = {c: flatten_sets(hbit[c], hsnp[c], order[c]) for c in chrom_lst if hsnp.get(c)}
    dup = sum(s.duplicates for s in out.values())
    if dup:
        print("himut haplotag: {} positions of {} are listed twice: the record that stands first in the file is kept".format(
            dup, vcf_file))
    return out, absent


def format_reads(chrom, rows, info, names, name_of):
    """The lines (no header) of one contig's reads: ``rows`` as Context.haplotag returns them, ``info`` = (tstart, tend,
    flag, mapq) per read, ``names`` the sets' PS strings, ``name_of(read ordinal)`` the read's name."""
    from ._ffi import HAPLOTAG_STATUS_NAMES
    tstart, tend, flag, mapq = info
    out = []
    for r in rows:
        i, s, hap = int(r["read"]), int(r["set"]), int(r["hap"])
        out.append("{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}".format(
            chrom, name_of(i), int(tstart[i]) + 1, int(tend[i]), "-" if int(flag[i]) & 0x10 else "+", int(mapq[i]),
            names[s] if s >= 0 else ".", hap + 1 if hap < 2 else ".", HAPLOTAG_STATUS_NAMES[int(r["status"])], int(r["n0"]),
            int(r["n1"]), int(r["n_other"]), int(r["n_del"]), int(r["n_lowbq"]), int(r["n_sets"])))
    return out


def format_snps(chrom, snps, snp_rows):
    """The lines (no header) of one contig's hetSNPs: ``snps`` a PhasedSnps, ``snp_rows`` as Context.haplotag returns them."""
    out = []
    for (pos, ref, alt, bit, s), r in zip(snps.tuples(), snp_rows):
        counts = [int(r[k]) for k in ("n_ref", "n_alt", "n_other", "n_del", "n_lowbq")]
        out.append("\t".join(str(x) for x in [chrom, pos, ref, alt, "1|0" if bit else "0|1", snps.names[s], sum(counts)] + counts +
                             [int(r["agree"]), int(r["disagree"])]))
    return out


def log_of(log, snp_rows):
    """The sixteen rows of himut_haplotag.log for one contig: the run's counters, the hetSNPs, those with a spanning pile
    read and those more assigned reads disagree with than agree."""
    depth = sum(snp_rows[k].astype(np.int64) for k in ("n_ref", "n_alt", "n_other", "n_del", "n_lowbq")) if len(snp_rows) else np.zeros(0)
    return [int(x) for x in log] + [len(snp_rows), int(np.sum(depth > 0)), int(np.sum(snp_rows["disagree"] > snp_rows["agree"]))]


def get_haplotags(chrom, bam_file, snps, min_mapq, min_bq, min_snps, min_agree_permille, chrom2out, device=0, read_batch=None,
                  resident_worker=None):
    """One contig (the shape of support.get_support_rows): its reads from ``read_batch``, from ``bam_file`` with the
    package's BAM reader, or already in HBM under ``resident_worker``.  ``snps``: the contig's PhasedSnps.
    chrom2out[chrom] = (rows, hetSNP rows, the thirteen counters, (tstart, tend, flag, mapq) of the reads)."""
    w, read_batch = reads_for(resident_worker, read_batch, bam_file, chrom, device)
    if read_batch is not None:
        w.ctx.push_reads(read_batch)
    w.ctx.run_haplotag(snps.pos1, snps.ref, snps.alt, snps.bit, snps.set, n_sets=len(snps.names), min_mapq=min_mapq, min_bq=min_bq,
                       min_snps=min_snps, min_agree_permille=min_agree_permille)
    rows, snp_rows, log = w.ctx.haplotag()
    chrom2out[chrom] = (rows, snp_rows, log, w.ctx.read_info(len(rows)))


def dump_haplotags(bam_file, phased_vcf_file, region, region_list, min_mapq, min_bq, min_snps, min_agree_permille, threads, out_file,
                   snps_file=None, devices=(0,), ref_file=None, cs_from_ref=False, log_file="himut_haplotag.log"):
    """Driver of `himut haplotag`: the phased VCF's hetSNPs, every target contig the VCF names through the device-side
    ingest (one resident context per contig, contigs spread over ``devices``, the reads' names kept on the host), the
    TSV per read, with ``snps_file`` the TSV per hetSNP, and the counters.  ``cs_from_ref``: the BAM needs no cs tags,
    the ingest derives the text from CIGAR, SEQ and ``ref_file``.  A single process: under torch.distributed.run it
    raises."""
    import contextlib
    import time
    from . import _ffi, dist, util, vcflib
    from .feed import ContigFeed
    dist.require_single_process("haplotag", dist.DEVICES_HINT)
    _ffi.lib()                                  # no CPU implementation: raises here without the HIP library
    t0 = time.time()
    feed = ContigFeed(bam_file, region, region_list, threads, devices)
    chrom2snps, absent = load_phased(phased_vcf_file, feed.chrom_lst, feed.tname2tsize)
    for chrom in util.natsorted(absent):
        print("himut haplotag: contig {} of {} is not in {}: its {} hetSNPs are skipped".format(
            chrom, phased_vcf_file, bam_file, absent[chrom]))
    chrom_lst = [c for c in feed.chrom_lst if c in chrom2snps]
    if cs_from_ref:
        feed.derive_cs_from(ref_file, chrom_lst)
    device_of = dict(feed.share(chrom_lst))
    chrom2log = {}
    # one contig at a time, in the order of the output: its lines are written before the next contig is ingested
    with contextlib.ExitStack() as files, feed:
        reads_fh = files.enter_context(open(out_file, "w"))
        snps_fh = files.enter_context(open(snps_file, "w")) if snps_file else None
        reads_fh.write("\t".join(READ_COLUMNS) + "\n")
        if snps_fh:
            snps_fh.write("\t".join(SNP_COLUMNS) + "\n")
        for chrom in chrom_lst:
            dev = device_of[chrom]
            w, _res = feed.ingest(chrom, dev, keep_names=True)
            out = {}
            get_haplotags(chrom, bam_file, chrom2snps[chrom], min_mapq, min_bq, min_snps, min_agree_permille, out, device=dev,
                          resident_worker=w)
            rows, snp_rows, log, info = out[chrom]
            reads_fh.writelines(x + "\n" for x in format_reads(chrom, rows, info, chrom2snps[chrom].names, feed.bam.read_name))
            if snps_fh:
                snps_fh.writelines(x + "\n" for x in format_snps(chrom, chrom2snps[chrom], snp_rows))
            chrom2log[chrom] = log_of(log, snp_rows)
            feed.release(chrom)                 # the contig's reads leave HBM
    vcflib.dump_counter_log(LOG_ROWS, chrom_lst, chrom2log, log_file)
    print("himut haplotag took {} minutes".format((time.time() - t0) / 60))
    return chrom_lst
