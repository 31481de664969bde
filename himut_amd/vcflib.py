"""Side-VCF loaders and the himut VCF / log writers (reference:
src/himut/vcflib.py).  These stay in Python by design: the
device returns integers, and dividing / formatting them with the same Python
float formatting the reference uses makes the text identical by construction.

Behaviours reproduced on purpose (they change the output):
* load_common_snp keeps records of every contig EXCEPT the requested one,
  keyed by position only (vcflib.py:434).
* load_pon indexes column 10 of every record, so PoN files need a sample column
  (vcflib.py:26).
* the header prints max_mismatch_count under --mismatch_window and vice versa,
  because the driver passes them swapped (caller.py:742-743 vs vcflib.py:167-168).
"""
from collections import defaultdict
from datetime import datetime

from .util import natsorted

LOG_ROWS = ["num_ccs", "num_sbs", "num_het_sbs", "num_hetalt_sbs", "num_homalt_sbs", "num_somrev_sbs",
            "num_homref_sbs", "num_uncallable_sbs", "num_low_gq_sbs", "num_low_bq_sbs", "num_pon_filtered_sbs",
            "num_pop_filtered_sbs", "num_md_filtered_sbs", "num_ab_filtered_sbs", "num_som"]


class VcfRecord:
    """Fields of one VCF data line that the path looks at (vcflib.py:13-52)."""

    __slots__ = ("chrom", "pos", "ref", "alt_lst", "alt", "qual", "is_pass", "is_biallelic", "is_snp", "is_indel",
                 "sample_gt", "sample_phase_set")

    def __init__(self, line):
        f = line.strip().split()
        self.chrom = f[0]
        self.pos = int(f[1])
        self.ref = f[3]
        self.alt_lst = f[4].split(",")
        self.qual = float(f[5]) if f[5] != "." else f[5]       # printed back with str() by the phased-hetSNP writer
        self.is_pass = f[6] == "PASS"
        fmt = dict(zip(f[8].split(":"), f[9].split(":")))   # IndexError without a sample column, as the reference
        self.sample_gt = fmt.get("GT")
        self.sample_phase_set = fmt.get("PS")
        self.is_biallelic = len(self.alt_lst) == 1
        self.alt = self.alt_lst[0] if self.is_biallelic else None
        self.is_snp = self.is_biallelic and len(self.ref) == 1 and len(self.alt) == 1
        # vcflib.py:41-50: a doublet substitution is neither; anything else of unequal length is an indel
        self.is_indel = (self.is_biallelic and not self.is_snp and not (len(self.ref) == len(self.alt) == 2)
                         and len(self.ref) != len(self.alt))


def _data_lines(path):
    with open(path) as fh:
        for line in fh:
            if not line.startswith("#"):
                yield line


_SIDE_CACHE = {}


def _by_contig(vcf_file, kind, parse):
    """The records of a side VCF that pass ``parse`` (a line -> (chrom, key) or None), grouped by contig.  The reference
    reads the whole file again for every contig (its workers are separate processes); here one driver process asks for
    contig after contig, and the file is parsed once per (path, size, time of modification)."""
    import os
    st = os.stat(vcf_file)
    key = (os.path.abspath(vcf_file), kind, st.st_size, st.st_mtime_ns)
    hit = _SIDE_CACHE.get(key)
    if hit is None:
        hit = defaultdict(set)
        for line in _data_lines(vcf_file):
            r = parse(line)
            if r is not None:
                hit[r[0]].add(r[1])
        for k in [k for k in _SIDE_CACHE if k[:2] == key[:2]]:
            del _SIDE_CACHE[k]                      # an older version of the same file
        _SIDE_CACHE[key] = hit
    return hit


def _pon_record(line):
    v = VcfRecord(line)
    return (v.chrom, (v.pos, v.ref, v.alt)) if v.is_snp and v.is_pass else None


def load_pon(chrom, vcf_file):
    """(pos, ref, alt) of PASS bi-allelic SNVs on ``chrom`` (vcflib.py:396-409)."""
    return set(_by_contig(vcf_file, "pon", _pon_record).get(chrom, ()))


def _bgz_lines(path, chrom):
    """Data lines of a bgzip-compressed VCF on ``chrom``.  A BGZF file is a series of gzip members, so python's
    gzip reads it; the reference goes through a tabix index (vcflib.py:381,417,449), which only selects the same
    lines faster.  The region arguments of the reference's per-chunk queries (chunk +- qlen_upper_limit,
    caller.py:269-289) always contain the chunk, so one pass per contig gives the same membership answers."""
    import gzip
    with gzip.open(path, "rt") as fh:
        for line in fh:
            if line.startswith("#"):
                continue
            if line.split("\t", 1)[0] == chrom:
                yield line


def load_bgz_pon(chrom, vcf_file):
    """.bgz panel of normals on ``chrom`` (vcflib.py:412-423)."""
    out = set()
    for line in _bgz_lines(vcf_file, chrom):
        v = VcfRecord(line)
        if v.is_snp and v.is_pass:
            out.add((v.pos, v.ref, v.alt))
    return out


def load_bgz_common_snp(chrom, vcf_file):
    """.bgz common SNPs on ``chrom`` -- the tabix variant queries the RIGHT contig, unlike load_common_snp
    (vcflib.py:443-459)."""
    out = set()
    for line in _bgz_lines(vcf_file, chrom):
        f = line.strip().split("\t")
        alts = f[4].split(",")
        if f[6] == "PASS" and len(alts) == 1 and len(f[3]) == 1 and len(alts[0]) == 1:
            out.add((int(f[1]), f[3], alts[0]))
    return out


def _common_record(line):
    f = line.strip().split()
    alts = f[4].split(",")
    if f[6] == "PASS" and len(alts) == 1 and len(f[3]) == 1 and len(alts[0]) == 1:
        return f[0], (int(f[1]), f[3], alts[0])
    return None


def load_common_snp(chrom, vcf_file):
    """(pos, ref, alt) of PASS bi-allelic SNVs -- from the OTHER contigs
    (vcflib.py:426-440: ``if chrom != arr[0] and ...``)."""
    out = set()
    for c, keys in _by_contig(vcf_file, "common", _common_record).items():
        if c != chrom:
            out |= keys
    return out


def load_phased_hetsnps(vcf_file, chrom_lst, tname2tsize):
    """Phase sets of 0|1 / 1|0 records (vcflib.py:617-663).  Returns
    (chrom2ps2hbit, chrom2ps2hpos, chrom2ps2hetsnp, chrom2chunkloci); the chunk
    list becomes one (chrom, first_pos, last_pos) per phase set."""
    hbit = {t: defaultdict(list) for t in tname2tsize}
    hpos = {t: defaultdict(list) for t in tname2tsize}
    hsnp = {t: defaultdict(list) for t in tname2tsize}
    # a plain .vcf is read whole, a .bgz contig by contig in the order asked for (the reference's tabix queries)
    for _, v in _hetsnp_lines(vcf_file, chrom_lst):
        if v.sample_gt in ("0|1", "1|0"):
            if v.alt is None:
                raise AttributeError("multi-allelic phased record (the reference fails here too)")
            hpos[v.chrom][v.sample_phase_set].append(v.pos)
            hsnp[v.chrom][v.sample_phase_set].append((v.pos, v.ref, v.alt))
            hbit[v.chrom][v.sample_phase_set].append(v.sample_gt.split("|")[0])
    wanted = set(chrom_lst)
    chunks = {}
    for t in list(tname2tsize):
        if t not in wanted:
            del hbit[t], hpos[t], hsnp[t]
            continue
        chunks[t] = [(t, p[0], p[-1]) for p in hpos[t].values()]
    return hbit, hpos, hsnp, chunks


def phased_record_order(vcf_file):
    """Of a phased VCF, plain .vcf or .bgz, in one pass over the file: contig -> {(pos, PS): the number of the first data
    line that lists the position in that phase set}, for the 0|1 / 1|0 records load_phased_hetsnps keeps.  It says what
    that function's dicts, keyed by phase set, cannot: which of two records of different sets stands first in the file,
    and which contigs the file names (a .bgz is otherwise read for the contigs asked for only).  A line without a sample
    column is passed over here; load_phased_hetsnps raises on it where it reads it."""
    import gzip
    order = {}
    with (gzip.open(vcf_file, "rt") if vcf_file.endswith(".bgz") else open(vcf_file)) as fh:
        k = 0
        for line in fh:
            if line.startswith("#"):
                continue
            k += 1
            f = line.split()
            if len(f) < 10:
                continue
            fmt = dict(zip(f[8].split(":"), f[9].split(":")))
            if fmt.get("GT") in ("0|1", "1|0"):
                order.setdefault(f[0], {}).setdefault((int(f[1]), fmt.get("PS")), k)
    return order


# --------------------------------------------------------------------------------------
# header (vcflib.py:150-353)

_FILTERS = [
    ("PASS", "All filters passed"),
    ("LowBQ", "Base quality score is below the minimum base quality score of {min_bq}"),
    ("LowGQ", "Germline genotype quality score is below the minimum genotype quality score of {min_gq}"),
    ("IndelSite", "Somatic substitution at indel site is not considered"),
    ("HetSite", "Somatic substitution at heterzygous SNP site is not considered"),
    ("HetAltSite", "Somatic substitution at tri-allelic SNP site is not considered"),
    ("HomAltSite", "Somatic substitution at homozygous alternative SNP site is not considered"),
    ("ComSnp", "Substitution is potentially from genomic DNA contamination"),
    ("PanelOfNormal", "Substitution is found within the Panel of Normal VCF file"),
    ("LowDepth", "Read depth is below the minimum reference allele and/or alterantive allele depth threshold"),
    ("HighDepth", "Read depth is above the maximum depth threshold of {md_threshold:.1f}"),
    ("Trimmed", "Substitution is positioned near the end of reads"),
    ("MismatchConflict", "Substitution is found next to a mismatch within a given mismatch window"),
    ("Unphased", "CCS read is not haplotype phased"),
]
_FORMATS = [
    ("GT", "1", "String", "Genotype"),
    ("GQ", "1", "String", "Genotype quality score"),
    ("BQ", "1", "Float", "Base quality score"),
    ("DP", "1", "Integer", "Read depth"),
    ("AD", "R", "Integer", "Read depth for each allele"),
    ("VAF", "A", "Float", "Variant allele fractions"),
    ("PS", "1", "Integer", "Phase set"),
]


def _region_param(region, region_list):
    if region_list is not None:
        return "--region_list {}".format(region_list)
    if region is not None:
        return "--region {}".format(region)
    return ""


def _options(opts):
    return "".join(" {} {}".format(k, v) for k, v in opts)


def _column_line(sample):
    return "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t{}".format(sample)


def _vcf_header(content, extra, filters, limits, formats, tname2tsize, command, version, sample):
    """The header every command's VCF has: the preamble up to ``##content=``, the ``extra`` lines, a FILTER line per row
    of ``filters`` (ID, description with the ``limits`` filled in), a FORMAT line per row of ``formats``, the contigs in
    natural order, ``##himut_command=`` + ``command`` and the column line with the sample."""
    lines = ["##fileformat=VCFv4.2", "##fileDate={}".format(datetime.now().strftime("%d%m%Y")), "##source=himut",
             "##source_version={}".format(version), "##content={}".format(content)]
    lines += extra
    lines += ['##FILTER=<ID={},Description="{}">'.format(fid, desc.format(**limits)) for fid, desc in filters]
    lines += ['##FORMAT=<ID={},Number={},Type={},Description="{}">'.format(*row) for row in formats]
    lines += ["##contig=<ID={},length={}>".format(tname, tname2tsize[tname]) for tname in natsorted(list(tname2tsize.keys()))]
    lines += ["##himut_command={}".format(command), _column_line(sample)]
    return "\n".join(lines)


def _run_command(sub, bam_file, ref_file, region, region_list, opts, cs_from_ref):
    """The command line of the runs added here (germline, dbs, indels): ``--ref`` when a FASTA was given, the region, the
    options, ``--cs_from_ref`` last."""
    return "himut {} -i {}{} {}{}{}".format(sub, bam_file, "" if ref_file is None else " --ref {}".format(ref_file),
                                            _region_param(region, region_list), _options(opts),
                                            " --cs_from_ref" if cs_from_ref else "")


def get_himut_vcf_header(bam_file, vcf_file, phased_vcf_file, region, region_list, tname2tsize, common_snps,
                         panel_of_normals, min_qv, min_mapq, qlen_lower_limit, qlen_upper_limit,
                         min_sequence_identity, min_gq, min_bq, min_trim, mismatch_window, max_mismatch_count,
                         md_threshold, min_ref_count, min_alt_count, min_hap_count, threads, somatic_snv_prior,
                         germline_snv_prior, germline_indel_prior, phase, non_human_sample, reference_sample,
                         create_panel_of_normals, version, out_file, sample):
    """Same positional meaning as vcflib.get_himut_vcf_header plus the sample
    name (the reference reads it from the BAM @RG line, bamlib.py:89-106)."""
    opts = [("--min_qv", min_qv), ("--min_mapq", min_mapq), ("--qlen_lower_limit", qlen_lower_limit),
            ("--qlen_upper_limit", qlen_upper_limit), ("--min_sequence_identity", min_sequence_identity),
            ("--min_gq", min_gq), ("--min_bq", min_bq), ("--min_trim", min_trim),
            ("--mismatch_window", mismatch_window), ("--max_mismatch_count", max_mismatch_count),
            ("--min_ref_count", min_ref_count), ("--min_alt_count", min_alt_count)]
    if phase:
        opts.append(("--min_hap_count", min_hap_count))
    opts += [("--somatic_snv_prior", somatic_snv_prior), ("--germline_snv_prior", germline_snv_prior),
             ("--germline_indel_prior", germline_indel_prior), ("--threads", threads), ("-o", out_file)]
    param = _region_param(region, region_list) + _options(opts)

    head = "himut call -i {}".format(bam_file)
    cmd = None
    if phase and non_human_sample:
        cmd = "{} --vcf {} --phased_vcf {} {} --phase --non_human_sample{}".format(
            head, vcf_file, phased_vcf_file, param, " --reference_sample" if reference_sample else "")
    elif phase and not non_human_sample and not reference_sample:
        cmd = "{} --phased_vcf {} {} --common_snps {} --panel_of_normals {} --phase".format(
            head, phased_vcf_file, param, common_snps, panel_of_normals)
    elif not phase and non_human_sample and not create_panel_of_normals:
        cmd = "{} --vcf {} {} --non_human_sample{}".format(
            head, vcf_file, param, " --reference_sample" if reference_sample else "")
    elif not phase and not non_human_sample and not reference_sample and create_panel_of_normals:
        cmd = "{} --vcf {} {} --create_panel_of_normals".format(head, vcf_file, param)
    elif not phase and not non_human_sample and not reference_sample:
        cmd = "{} --vcf {} {} --common_snps {} --panel_of_normals {}".format(
            head, vcf_file, param, common_snps, panel_of_normals)
    if cmd is None:
        raise UnboundLocalError("flag combination has no command line in the reference header builder")
    return _vcf_header("himut somatic single base substitutions", [], _FILTERS,
                       dict(min_bq=min_bq, min_gq=min_gq, md_threshold=md_threshold), _FORMATS, tname2tsize, cmd, version, sample)


# --------------------------------------------------------------------------------------
# writers (vcflib.py:820-1060)

def _body_line(rec, phased, single_molecule_file):
    chrom, pos, ref, alt, status, gq, bq, depth, ref_count, alt_count, vaf, ps = rec
    if status == "HetAltSite":
        # bq / alt_count / vaf arrive pre-formatted (caller.py:174-192).  In the
        # phased main file the FORMAT column of this line lacks ":PS" although
        # the sample column has it (vcflib.py:954).
        fmt = "GT:GQ:BQ:DP:AD:VAF:PS" if (phased and single_molecule_file) else "GT:GQ:BQ:DP:AD:VAF"
        sample = "./.:{}:{}:{:0.0f}:{:0.0f},{}:{}".format(gq, bq, depth, ref_count, alt_count, vaf)
    else:
        fmt = "GT:GQ:BQ:DP:AD:VAF:PS" if phased else "GT:GQ:BQ:DP:AD:VAF"
        sample = "./.:{}:{:0.1f}:{:0.0f}:{:0.0f},{:0.0f}:{:.2f}".format(gq, bq, depth, ref_count, alt_count, vaf)
    if phased:
        sample += ":{}".format(ps)
    return "{}\t{}\t.\t{}\t{}\t.\t{}\t.\t{}\t{}\n".format(chrom, pos, ref, alt, status, fmt, sample)


def _dump(vcf_file, vcf_header, chrom_lst, chrom2tsbs_lst, phased):
    if not vcf_file.endswith(".vcf"):
        raise ValueError("VCF file must have .vcf suffix")
    with open(vcf_file, "w") as main, open(vcf_file.replace(".vcf", ".single_molecule_mutations.vcf"), "w") as sm:
        main.write("{}\n".format(vcf_header))
        sm.write("{}\n".format(vcf_header))
        for chrom in chrom_lst:
            for rec in chrom2tsbs_lst[chrom]:
                main.write(_body_line(rec, phased, False))
                # single-molecule file: one supporting read (vcflib.py:868,896)
                single = int(rec[8]) == 1 if rec[4] == "HetAltSite" else int(rec[9]) == 1
                if single:
                    sm.write(_body_line(rec, phased, True))


def dump_records(vcf_file, vcf_header, chrom_lst, chrom2recs, phased):
    """The same two files straight from the integer records (numpy arrays of RECORD_DTYPE), formatted by the host
    library: what dump_sbs / dump_phased_sbs write for caller.records_to_tuples(chrom, recs)."""
    from . import bamio
    if not vcf_file.endswith(".vcf"):
        raise ValueError("VCF file must have .vcf suffix")
    with open(vcf_file, "wb") as main, open(vcf_file.replace(".vcf", ".single_molecule_mutations.vcf"), "wb") as sm:
        main.write("{}\n".format(vcf_header).encode())
        sm.write("{}\n".format(vcf_header).encode())
        for chrom in chrom_lst:
            main.write(bamio.format_records(chrom2recs[chrom], chrom, phased, False))
            sm.write(bamio.format_records(chrom2recs[chrom], chrom, phased, True))


def dump_sbs(vcf_file, vcf_header, chrom_lst, chrom2tsbs_lst):
    _dump(vcf_file, vcf_header, chrom_lst, chrom2tsbs_lst, False)


def dump_phased_sbs(vcf_file, vcf_header, chrom_lst, chrom2tsbs_lst):
    _dump(vcf_file, vcf_header, chrom_lst, chrom2tsbs_lst, True)


def dump_vcf(vcf_file, vcf_header, chrom_lst, lines_of):
    """A one-file VCF: the header, then ``lines_of(chrom)`` (a list of data lines) contig by contig."""
    if not vcf_file.endswith(".vcf"):
        raise ValueError("VCF file must have .vcf suffix")
    with open(vcf_file, "w") as o:
        o.write("{}\n".format(vcf_header))
        for chrom in chrom_lst:
            o.writelines(lines_of(chrom))


def dump_counter_log(rows, chrom_lst, chrom2log, path):
    """A counter table in the layout of himut.log (vcflib.py:1024-1060): a column per contig and their total, a row per
    name of ``rows``; chrom2log[chrom][k] is the count of rows[k]."""
    with open(path, "w") as o:
        o.write("{:30}{}\n".format("", "\t".join(list(chrom_lst) + ["total"])))
        for k, name in enumerate(rows):
            cells = [int(chrom2log[chrom][k]) for chrom in chrom_lst]
            o.write("{:30}{}\n".format(name, "\t".join(str(x) for x in cells + [sum(cells)])))


def dump_call_log(chrom_lst, chrom2tsbs_log, path="himut.log"):
    """`call`'s counter table, written to ./himut.log."""
    dump_counter_log(LOG_ROWS, chrom_lst, chrom2tsbs_log, path)


# --------------------------------------------------------------------------
# `himut phase`: hetSNP input and the phased-hetSNP VCF (vcflib.py:84-147,462-550,704-817)

def _is_het_snp(v):
    return v.is_snp and v.is_pass and v.is_biallelic and v.sample_gt in ("0/1", "1/0")


def _hetsnp_lines(vcf_file, chrom_lst):
    """(line, record) of every data line the phaser looks at: the whole plain .vcf in file order, or the requested
    contigs of a .bgz one after the other (what the reference's tabix queries return)."""
    if vcf_file.endswith(".vcf"):
        for line in _data_lines(vcf_file):
            yield line, VcfRecord(line)
    elif vcf_file.endswith(".bgz"):
        for chrom in chrom_lst:
            for line in _bgz_lines(vcf_file, chrom):
                yield line, VcfRecord(line)


def load_hetsnps(vcf_file, chrom, chrom_len):
    """PASS bi-allelic 0/1 SNPs of ``chrom`` in file order: (hetsnp_lst, hidx2hetsnp, hetsnp2hidx)
    (vcflib.py:462-499)."""
    hetsnp_lst = [(v.pos, v.ref, v.alt) for _, v in _hetsnp_lines(vcf_file, [chrom]) if v.chrom == chrom and _is_het_snp(v)]
    hidx2hetsnp = dict(enumerate(hetsnp_lst))
    hetsnp2hidx = {h: i for i, h in hidx2hetsnp.items()}
    return hetsnp_lst, hidx2hetsnp, hetsnp2hidx


def load_hblock_hsh(vcf_file, chrom_lst, tname2tsize, chrom2hblock_lst):
    """hetSNP -> haplotype state and hetSNP -> phase set (= position of the block's first hetSNP) for every
    hetSNP a block holds (vcflib.py:502-550).  Keys carry no contig, as in the reference: the same (pos, ref, alt)
    on two contigs share an entry."""
    per_chrom = defaultdict(list)
    for _, v in _hetsnp_lines(vcf_file, chrom_lst):
        if _is_het_snp(v):
            per_chrom[v.chrom].append((v.pos, v.ref, v.alt))
    hetsnp2hstate, hetsnp2phase_set = {}, {}
    for chrom, hblock_lst in chrom2hblock_lst.items():
        snps = per_chrom[chrom]
        for hblock in hblock_lst:
            phase_set = snps[hblock[0][0]][0]
            for hidx, hstate in hblock:
                hetsnp2hstate[snps[hidx]] = hstate
                hetsnp2phase_set[snps[hidx]] = phase_set
    return hetsnp2hstate, hetsnp2phase_set


def get_phased_vcf_header(bam_file, vcf_file, region, region_list, tname2tsize, min_bq, min_mapq, min_p_value,
                          min_phase_proportion, threads, version, out_file, sample):
    """Header of the phased-hetSNP VCF (vcflib.py:84-147); ``sample`` is the BAM's SM tag."""
    h = ["##fileformat=VCFv4.2",
         '##FILTER=<ID=PASS,Description="All filters passed">',
         "##fileDate={}".format(datetime.now().strftime("%d%m%Y")),
         "##source=himut",
         "##source_version={}".format(version),
         "##content=himut somatic single base substitutions",
         '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
         '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Conditional genotype quality">',
         '##FORMAT=<ID=BQ,Number=1,Type=Float,Description="Average base quality">',
         '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Read depth">',
         '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Read depth for each allele">',
         '##FORMAT=<ID=VAF,Number=A,Type=Float,Description="Variant allele fractions">',
         '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods rounded to the closest integer">',
         '##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase set">']
    h += ["##contig=<ID={},length={}>".format(t, tname2tsize[t]) for t in natsorted(list(tname2tsize))]
    h.append("##himut_command=himut phase -i {} --vcf {} {} --min_bq {} --min_mapq {} --min_p_value {} "
             "--min_phase_proportion {} --threads {} -o {}".format(bam_file, vcf_file, _region_param(region, region_list), min_bq,
                                                                   min_mapq, min_p_value, min_phase_proportion, threads, out_file))
    h.append(_column_line(sample))
    return "\n".join(h)


def dump_phased_hetsnps(bam_file, vcf_file, region, region_list, tname2tsize, min_bq, min_mapq, min_p_value,
                        min_phase_proportion, threads, chrom_lst, chrom2hblock_lst, version, out_file, sample):
    """The input's hetSNPs again, with GT 0|1 / 1|0 and PS for those inside a block and PS "." for the others
    (vcflib.py:704-817).  The plain-.vcf branch prints the hetSNPs of every contig of the file, the .bgz branch
    those of the requested contigs."""
    hetsnp2hstate, hetsnp2phase_set = load_hblock_hsh(vcf_file, chrom_lst, tname2tsize, chrom2hblock_lst)
    with open(out_file, "w") as o:
        o.write("{}\n".format(get_phased_vcf_header(bam_file, vcf_file, region, region_list, tname2tsize, min_bq, min_mapq,
                                                    min_p_value, min_phase_proportion, threads, version, out_file, sample)))
        for line, v in _hetsnp_lines(vcf_file, chrom_lst):
            if not _is_het_snp(v):
                continue
            fmt, sample_fmt = line.strip().split()[-2:]
            hetsnp = (v.pos, v.ref, v.alt)
            if hetsnp in hetsnp2hstate:
                cols = sample_fmt.split(":")
                cols[0] = "0|1" if hetsnp2hstate[hetsnp] == "0" else "1|0"
                tail = "{}:{}".format(":".join(cols), hetsnp2phase_set[hetsnp])
            else:
                tail = "{}:.".format(sample_fmt)
            o.write("{}\t{}\t.\t{}\t{}\t{}\tPASS\t.\t{}:PS\t{}\n".format(v.chrom, v.pos, v.ref, v.alt, v.qual, fmt, tail))


# --------------------------------------------------------------------------
# --non_human_sample: germline priors from the sample's own VCF (vcflib.py:553-613)

def load_germline_counts(vcf_file, chrom_lst):
    """(het SNPs, hom-alt SNPs, het indels, hom-alt indels) among the PASS bi-allelic records of the target contigs;
    only the genotype spellings 0/1 and 1/1 count (vcflib.py:553-593).  A .vcf.bgz is read as the gzip members it
    is made of (the reference goes through cyvcf2)."""
    import gzip
    if vcf_file.endswith(".vcf"):
        fh = open(vcf_file)
    elif vcf_file.endswith(".vcf.bgz"):
        fh = gzip.open(vcf_file, "rt")
    else:
        return 0, 0, 0, 0
    n = defaultdict(int)
    with fh:
        for line in fh:
            if line.startswith("#"):
                continue
            v = VcfRecord(line)
            if v.is_pass and v.is_biallelic and v.sample_gt in ("0/1", "1/1") and (v.is_snp or v.is_indel):
                n[(v.chrom, v.is_snp, v.sample_gt)] += 1
    tot = lambda snp, gt: sum(n[(c, snp, gt)] for c in chrom_lst)
    return tot(True, "0/1"), tot(True, "1/1"), tot(False, "0/1"), tot(False, "1/1")


def get_germline_priors(chrom_lst, ref_file, vcf_file, reference_sample):
    """Germline SNV and indel priors = variants per base of the target contigs, truncated to their first
    significant digit (vcflib.py:596-613): a reference sample counts its het sites twice, any other sample its
    het and hom-alt sites once."""
    from .normcounts import read_fasta
    from .util import get_truncated_float
    refseq = read_fasta(ref_file)
    target_sum = sum(len(refseq[chrom]) for chrom in chrom_lst)
    hetsnp, homsnp, hetindel, homindel = load_germline_counts(vcf_file, chrom_lst)
    if reference_sample:
        snv, indel = (2 * hetsnp) / target_sum, (2 * hetindel) / target_sum
    else:
        snv, indel = (hetsnp + homsnp) / target_sum, (hetindel + homindel) / target_sum
    return get_truncated_float(snv), get_truncated_float(indel)


# --------------------------------------------------------------------------
# `himut germline`: the sample's het, hom-alt and het-alt SNVs from the call path's pile.  The reference has no such
# command (it takes this file from an external caller); the lines are what its own loaders read (vcflib.py:13-52,
# 462-499, 553-593): `phase --vcf`, `call --phase` through phase's output, `--non_human_sample`.

GERMLINE_LOG_ROWS = ["num_pos", "num_nref", "num_homref", "num_het", "num_hetalt", "num_homalt", "num_pass", "num_low_gq",
                     "num_low_bq", "num_low_depth", "num_high_depth", "reserved"]

_GERMLINE_FILTERS = [
    ("PASS", "All filters passed"),
    ("LowGQ", "Genotype quality score below minimum genotype quality score threshold of {min_gq}"),
    ("LowBQ", "No read with base quality score of {min_bq} or above supports an alternative allele"),
    ("LowDepth", "Alternative allele depth below {min_alt_count}, or heterozygous and reference allele depth below "
                 "{min_ref_count}"),
    ("HighDepth", "Read depth is above the maximum depth threshold of {md_threshold}"),
]
_GERMLINE_FORMATS = [
    ("GT", "1", "String", "Genotype"),
    ("GQ", "1", "Integer", "Genotype quality"),
    ("DP", "1", "Integer", "Read depth"),
    ("AD", "R", "Integer", "Read depth for each allele"),
    ("VAF", "A", "Float", "Variant allele fractions"),
]
_GERMLINE_STATUS = {0: "PASS", 1: "LowBQ", 2: "LowGQ", 9: "LowDepth", 10: "HighDepth"}      # HIMUT_ST_*
_ALLELE_IDX = {"A": 0, "T": 1, "G": 2, "C": 3}


def get_germline_vcf_header(bam_file, region, region_list, tname2tsize, min_mapq, min_gq, min_bq, min_ref_count,
                            min_alt_count, md_threshold, germline_snv_prior, threads, version, out_file, sample,
                            ref_file=None, cs_from_ref=False):
    """Header of the germline VCF: the five FILTER lines, FORMAT lines for GT:GQ:DP:AD:VAF, the contigs, the command's
    parameters as `call`'s header records them, the sample name from the BAM."""
    opts = [("--min_mapq", min_mapq), ("--min_gq", min_gq), ("--min_bq", min_bq), ("--min_ref_count", min_ref_count),
            ("--min_alt_count", min_alt_count), ("--germline_snv_prior", germline_snv_prior), ("--threads", threads),
            ("-o", out_file)]
    return _vcf_header("himut germline single nucleotide variants", [], _GERMLINE_FILTERS,
                       dict(min_gq=min_gq, min_bq=min_bq, min_ref_count=min_ref_count, min_alt_count=min_alt_count,
                            md_threshold=md_threshold), _GERMLINE_FORMATS, tname2tsize,
                       _run_command("germline", bam_file, ref_file, region, region_list, opts, cs_from_ref), version, sample)


def germline_lines(chrom, recs):
    """The data lines of the germline records of one contig (RECORD_DTYPE; homref records are not printed):
    het ALT x, GT 0/1; homalt ALT x, GT 1/1; hetalt ALT x,y in genotype order, GT 1/2.  DP = A+T+G+C+del
    (bamlib.get_read_depth), AD = the reference allele's count, then each alt's, VAF = alt count / DP."""
    out = []
    for r in recs:
        state = int(r["gt_state"])
        if state == 0:
            continue
        c = [int(x) for x in r["counts"]]
        depth = c[0] + c[1] + c[2] + c[3] + c[5]
        ref = chr(r["ref"])
        g0, g1 = chr(r["gt0"]), chr(r["gt1"])
        if state == 1:
            alts, gt = [g1], "0/1"
        elif state == 3:
            alts, gt = [g0], "1/1"
        else:
            alts, gt = [g0, g1], "1/2"
        ad = [c[_ALLELE_IDX[ref]]] + [c[_ALLELE_IDX[a]] for a in alts]
        vaf = ",".join("{:.2f}".format(c[_ALLELE_IDX[a]] / depth) for a in alts)
        out.append("{}\t{}\t.\t{}\t{}\t{}\t{}\t.\tGT:GQ:DP:AD:VAF\t{}:{}:{}:{}:{}\n".format(
            chrom, int(r["tpos"]), ref, ",".join(alts), int(r["gq"]), _GERMLINE_STATUS[int(r["status"])], gt,
            int(r["gq"]), depth, ",".join(str(x) for x in ad), vaf))
    return out


# --------------------------------------------------------------------------
# `himut dbs`: doublet base substitutions

DBS_LOG_ROWS = ["num_ccs", "num_dbs_runs", "num_mbs", "num_trimmed", "num_mismatch_conflict", "num_dbs", "num_germ",
                "num_HetSite", "num_HetAltSite", "num_HomAltSite", "num_IndelSite", "num_LowGQ", "num_LowBQ",
                "num_PanelOfNormal", "num_ComSnp", "num_LowDepth", "num_HighDepth", "num_PASS", "reserved0", "reserved1"]


def get_dbs_vcf_header(bam_file, region, region_list, tname2tsize, common_snps, panel_of_normals, min_qv, min_mapq,
                       qlen_lower_limit, qlen_upper_limit, min_sequence_identity, min_gq, min_bq, min_trim,
                       max_mismatch_count, mismatch_window_size, md_threshold, min_ref_count, min_alt_count,
                       germline_snv_prior, threads, version, out_file, sample, ref_file=None, cs_from_ref=False):
    """`call`'s header (its content, FILTER, FORMAT and contig lines, the column line) with the command line of `himut
    dbs` in the place of `call`'s."""
    opts = [("--min_qv", min_qv), ("--min_mapq", min_mapq), ("--qlen_lower_limit", qlen_lower_limit),
            ("--qlen_upper_limit", qlen_upper_limit), ("--min_sequence_identity", min_sequence_identity),
            ("--min_gq", min_gq), ("--min_bq", min_bq), ("--min_trim", min_trim),
            ("--mismatch_window_size", mismatch_window_size), ("--max_mismatch_count", max_mismatch_count),
            ("--min_ref_count", min_ref_count), ("--min_alt_count", min_alt_count),
            ("--germline_snv_prior", germline_snv_prior), ("--threads", threads), ("-o", out_file),
            ("--common_snps", common_snps), ("--panel_of_normals", panel_of_normals)]
    return _vcf_header("himut somatic single base substitutions", [], _FILTERS,
                       dict(min_bq=min_bq, min_gq=min_gq, md_threshold=md_threshold), _FORMATS, tname2tsize,
                       _run_command("dbs", bam_file, ref_file, region, region_list, opts, cs_from_ref), version, sample)


def dbs_lines(chrom, recs):
    """The data lines of the doublet records of one contig (DBS_RECORD_DTYPE) in _body_line's format with two-letter REF
    and ALT: BQ = the alt quality sum of both columns over both alt counts, DP = the smaller half depth (A+T+G+C+del),
    AD = both_ref,both_alt, VAF = both_alt / DP."""
    from ._ffi import STATUS_NAMES
    out = []
    for r in recs:
        ref, alt = chr(r["ref"][0]) + chr(r["ref"][1]), chr(r["alt"][0]) + chr(r["alt"][1])
        c = [[int(x) for x in h] for h in r["counts"]]
        depth = float(min(h[0] + h[1] + h[2] + h[3] + h[5] for h in c))
        n_alt = c[0][_ALLELE_IDX[alt[0]]] + c[1][_ALLELE_IDX[alt[1]]]
        bq = (int(r["alt_bqsum"][0]) + int(r["alt_bqsum"][1])) / float(n_alt) if n_alt else 0.0
        # _body_line's line for a single-base record (a doublet whose verdict is a half's HetAltSite is printed like every
        # other: its numbers are the joint counts)
        sample = "./.:{}:{:0.1f}:{:0.0f}:{:0.0f},{:0.0f}:{:.2f}".format(int(r["gq"]), bq, depth, float(r["both_ref"]),
                                                                      float(r["both_alt"]), int(r["both_alt"]) / depth)
        out.append("{}\t{}\t.\t{}\t{}\t.\t{}\t.\t{}\t{}\n".format(chrom, int(r["tpos"]), ref, alt, STATUS_NAMES[int(r["status"])],
                                                                     "GT:GQ:BQ:DP:AD:VAF", sample))
    return out


# --------------------------------------------------------------------------
# `himut indels`: germline short insertions and deletions

INDEL_LOG_ROWS = ["num_events", "num_alleles", "num_edge", "num_long", "num_nbase", "num_dup", "num_homref", "num_het",
                  "num_homalt", "num_pass", "num_low_gq", "num_low_depth", "num_high_depth"]
_INDEL_FILTERS = [
    ("PASS", "All filters passed"),
    ("LowGQ", "Genotype quality score below minimum genotype quality score threshold of {min_gq}"),
    ("LowDepth", "Fewer than {min_alt_count} reads carry the allele, or heterozygous and fewer than {min_ref_count} reads "
                 "do not"),
    ("HighDepth", "Read depth is above the maximum depth threshold of {md_threshold}"),
]
_INDEL_FORMATS = [
    ("GT", "1", "String", "Genotype"),
    ("GQ", "1", "Integer", "Genotype quality"),
    ("DP", "1", "Integer", "Reads that span the allele"),
    ("AD", "R", "Integer", "Reads without an indel at the anchor, reads with this allele"),
    ("NO", "1", "Integer", "Reads with another indel at the same anchor"),
]
_INDEL_CODES = "ATGC"


def get_indels_vcf_header(bam_file, region, region_list, tname2tsize, min_mapq, min_gq, min_ref_count, min_alt_count,
                          md_threshold, germline_indel_prior, indel_error, max_indel_len, threads, version, out_file, sample,
                          ref_file=None, cs_from_ref=False, error_table=None, min_spans=None):
    """Header of the indel VCF: the four FILTER lines, FORMAT lines for GT:GQ:DP:AD:NO, the contigs, the command's
    parameters, the sample name from the BAM.  Under ``error_table`` (--error_table) one more line, ##indel_error_table=,
    names the file and --min_spans; without it the header is what it was before the flag existed."""
    opts = [("--min_mapq", min_mapq), ("--min_gq", min_gq), ("--min_ref_count", min_ref_count),
            ("--min_alt_count", min_alt_count), ("--germline_indel_prior", germline_indel_prior),
            ("--indel_error", indel_error), ("--max_indel_len", max_indel_len), ("--threads", threads), ("-o", out_file)]
    extra = ["##alleles=left-normalised against the reference within each read; a multi-allelic anchor is written as one "
             "line per allele, NO counts the reads with another allele at the same anchor"]
    if error_table is not None:
        extra.append("##indel_error_table={} --min_spans {}: the per-read indel error of an allele in a homopolymer run is "
                     "its row's of this `himut indelcal` table, --indel_error elsewhere".format(error_table, min_spans))
    # (the command always names its FASTA, whatever ``ref_file`` is)
    return _vcf_header("himut germline short insertions and deletions", extra, _INDEL_FILTERS,
                       dict(min_gq=min_gq, min_ref_count=min_ref_count, min_alt_count=min_alt_count, md_threshold=md_threshold),
                       _INDEL_FORMATS, tname2tsize,
                       _run_command("indels", bam_file, str(ref_file), region, region_list, opts, cs_from_ref), version, sample)


def indel_lines(chrom, recs, chrom_seq):
    """The data lines of the indel records of one contig (INDEL_RECORD_DTYPE; homref records are not printed), REF and ALT
    from the contig's string, upper-cased: a deletion is REF = seq[a : a + 1 + L], ALT = seq[a]; an insertion REF = seq[a],
    ALT = seq[a] + the record's bases.  POS = a + 1, AD = n_ref,n_alt with n_ref = DP - n_alt - n_other (not below 0)."""
    out = []
    for r in recs:
        state = int(r["gt_state"])
        if state == 0:
            continue
        a, L = int(r["anchor"]), int(r["len"])
        if int(r["type"]) == 0:
            ref, alt = chrom_seq[a:a + 1 + L].upper(), chrom_seq[a].upper()
        else:
            b = r["bases"]
            ref = chrom_seq[a].upper()
            alt = ref + "".join(_INDEL_CODES[(int(b[i >> 2]) >> (2 * (i & 3))) & 3] for i in range(L))
        dp, n_alt, n_other = int(r["dp"]), int(r["n_alt"]), int(r["n_other"])
        out.append("{}\t{}\t.\t{}\t{}\t{}\t{}\t.\tGT:GQ:DP:AD:NO\t{}:{}:{}:{},{}:{}\n".format(
            chrom, a + 1, ref, alt, int(r["gq"]), _GERMLINE_STATUS[int(r["status"])], "0/1" if state == 1 else "1/1",
            int(r["gq"]), dp, max(0, dp - n_alt - n_other), n_alt, n_other))
    return out


# --------------------------------------------------------------------------
# `himut sindels`: somatic indel candidates carried by single reads

SINDEL_LOG_ROWS = ["num_events", "num_edge", "num_long", "num_nbase", "num_pile_reads", "num_proposing_reads",
                   "num_events_proposing_reads", "num_trim", "num_window", "num_lowbq", "num_proposing_events",
                   "num_candidates", "num_germ_het", "num_germ_homalt", "num_indel_site", "num_repeat", "num_low_gq",
                   "num_low_depth", "num_high_depth", "num_pass"]
_SINDEL_FILTERS = [
    ("PASS", "All filters passed"),
    ("IndelSite", "Another insertion or deletion is anchored at the same position"),
    ("Repeat", "A deletion inside a homopolymer run of the reference longer than {max_run}, or an insertion of its letter, "
               "or any allele in front of a run longer than 64; repeats of longer units are not recognised"),
    ("LowGQ", "Genotype quality score of the hom-ref pile below minimum genotype quality score threshold of {min_gq}"),
    ("LowDepth", "Fewer than {min_alt_count} reads carry the allele, or fewer than {min_ref_count} reads have no indel at "
                 "the anchor"),
    ("HighDepth", "Read depth is above the maximum depth threshold of {md_threshold}"),
]
_SINDEL_FORMATS = _INDEL_FORMATS + [("NP", "1", "Integer", "Reads whose event passed the read and event rules and proposed the allele")]
_SINDEL_INFOS = [
    ("RUN", "1", "String", "Letter and length of the homopolymer run of the reference that starts behind the anchor (65: longer than 64)"),
    ("CLASS", "1", "String", "Column of the allele in the `himut indelcal` table, where it has one"),
]
SINDEL_CLASS_NAMES = ("del1", "del2", "del3p", "ins1", "ins2", "ins3p", "other")


def get_sindels_vcf_header(bam_file, region, region_list, tname2tsize, min_qv, min_mapq, qlen_lower_limit, qlen_upper_limit,
                           min_sequence_identity, min_gq, min_bq, min_trim, max_mismatch_count, mismatch_window_size,
                           md_threshold, min_ref_count, min_alt_count, germline_indel_prior, indel_error, max_indel_len,
                           max_run, threads, version, out_file, sample, ref_file=None, cs_from_ref=False, error_table=None,
                           min_spans=None):
    """Header of the somatic indel VCF: the definitions the records rest on, the six FILTER lines, the INFO lines RUN and
    CLASS, FORMAT lines for GT:GQ:DP:AD:NO:NP, the contigs, the command's parameters, the sample name from the BAM."""
    opts = [("--min_qv", min_qv), ("--min_mapq", min_mapq), ("--qlen_lower_limit", qlen_lower_limit),
            ("--qlen_upper_limit", qlen_upper_limit), ("--min_sequence_identity", min_sequence_identity),
            ("--min_gq", min_gq), ("--min_bq", min_bq), ("--min_trim", min_trim),
            ("--mismatch_window_size", mismatch_window_size), ("--max_mismatch_count", max_mismatch_count),
            ("--min_ref_count", min_ref_count), ("--min_alt_count", min_alt_count),
            ("--germline_indel_prior", germline_indel_prior), ("--indel_error", indel_error),
            ("--max_indel_len", max_indel_len), ("--max_run", max_run), ("--threads", threads), ("-o", out_file)]
    extra = ["##candidates=not calls: HiFi indel error outside repeats is orders of magnitude above a somatic indel rate and "
             "higher still inside homopolymers; himut_sindels.log keeps the counters to subtract an expected error load "
             "from (`himut indelcal` gives the rate)",
             "##alleles=left-normalised against the reference within each read; a candidate is an allele that a read "
             "passing call's read filters shows with its footprint (the aligned base on either side and the inserted "
             "bases) untrimmed and at --min_bq and no more than --max_mismatch_count other mismatches in the window, in a "
             "pile that genotypes hom-ref (a het or hom-alt allele is dropped as germline)",
             "##definitions=--max_run, --indel_error and the footprint rule are definitions chosen here"]
    if error_table is not None:
        extra.append("##indel_error_table={} --min_spans {}: the per-read indel error of an allele in a homopolymer run is "
                     "its row's of this `himut indelcal` table, --indel_error elsewhere".format(error_table, min_spans))
    extra += ['##INFO=<ID={},Number={},Type={},Description="{}">'.format(*i) for i in _SINDEL_INFOS]
    return _vcf_header("himut somatic insertion and deletion candidates", extra, _SINDEL_FILTERS,
                       dict(min_gq=min_gq, min_ref_count=min_ref_count, min_alt_count=min_alt_count, md_threshold=md_threshold,
                            max_run=max_run),
                       _SINDEL_FORMATS, tname2tsize,
                       _run_command("sindels", bam_file, str(ref_file), region, region_list, opts, cs_from_ref), version, sample)


def sindel_lines(chrom, recs, chrom_seq):
    """The data lines of the candidate records of one contig (SINDEL_RECORD_DTYPE): REF, ALT and POS by indel_lines' rule,
    QUAL = gq, FILTER from the status, INFO RUN=<letter><n> where a run starts behind the anchor and CLASS=<column> where
    the allele has a class, GT:GQ:DP:AD:NO:NP with GT ./. (the pile is hom-ref; the allele is one molecule's)."""
    from ._ffi import SINDEL_STATUS_NAMES
    out = []
    for r in recs:
        a, L = int(r["anchor"]), int(r["len"])
        if int(r["type"]) == 0:
            ref, alt = chrom_seq[a:a + 1 + L].upper(), chrom_seq[a].upper()
        else:
            b = r["bases"]
            ref = chrom_seq[a].upper()
            alt = ref + "".join(_INDEL_CODES[(int(b[i >> 2]) >> (2 * (i & 3))) & 3] for i in range(L))
        info = []
        if int(r["run_len"]):
            info.append("RUN={}{}".format(_INDEL_CODES[int(r["run_base"])], int(r["run_len"])))
        if int(r["class_col"]) != 255:
            info.append("CLASS=" + SINDEL_CLASS_NAMES[int(r["class_col"])])
        dp, n_alt, n_other = int(r["dp"]), int(r["n_alt"]), int(r["n_other"])
        out.append("{}\t{}\t.\t{}\t{}\t{}\t{}\t{}\tGT:GQ:DP:AD:NO:NP\t./.:{}:{}:{},{}:{}:{}\n".format(
            chrom, a + 1, ref, alt, int(r["gq"]), SINDEL_STATUS_NAMES[int(r["status"])], ";".join(info) or ".",
            int(r["gq"]), dp, max(0, dp - n_alt - n_other), n_alt, n_other, int(r["n_prop"])))
    return out


# --------------------------------------------------------------------------
# `himut duplex`: substitutions on both strands of one molecule

_DUPLEX_INFOS = [
    ("DS", "1", "Integer", "Molecules whose two by-strand reads both show the substitution, each under call's read and event rules"),
    ("SS", "1", "Integer", "Reads of such pairs that show the substitution under those rules while the mate shows the reference base"),
    ("UNP", "1", "Integer", "Reads of the pile that show the substitution and are in no pair both of whose reads pass call's read filters"),
]
_DUPLEX_FORMATS = _FORMATS[:6] + _DUPLEX_INFOS
_DUPLEX_FILTERS = _FILTERS + [("Germline", "The germline genotype of the pile explains the allele (`call` drops such a candidate silently)")]


def get_duplex_vcf_header(bam_file, region, region_list, tname2tsize, common_snps, panel_of_normals, min_qv, min_mapq,
                          qlen_lower_limit, qlen_upper_limit, min_sequence_identity, min_gq, min_bq, min_trim,
                          max_mismatch_count, mismatch_window_size, md_threshold, min_ref_count, min_alt_count,
                          germline_snv_prior, threads, version, out_file, sample, ss_file=None, ref_file=None, cs_from_ref=False):
    """`call`'s header (its FILTER and contig lines, the column line) with what a double-strand record rests on, the INFO
    lines DS, SS and UNP, FORMAT lines for GT:GQ:BQ:DP:AD:VAF:DS:SS:UNP and the command line of `himut duplex`."""
    opts = [("--min_qv", min_qv), ("--min_mapq", min_mapq), ("--qlen_lower_limit", qlen_lower_limit),
            ("--qlen_upper_limit", qlen_upper_limit), ("--min_sequence_identity", min_sequence_identity),
            ("--min_gq", min_gq), ("--min_bq", min_bq), ("--min_trim", min_trim),
            ("--mismatch_window_size", mismatch_window_size), ("--max_mismatch_count", max_mismatch_count),
            ("--min_ref_count", min_ref_count), ("--min_alt_count", min_alt_count),
            ("--germline_snv_prior", germline_snv_prior), ("--threads", threads), ("-o", out_file)]
    if ss_file is not None:
        opts.append(("--ss", ss_file))
    opts += [("--common_snps", common_snps), ("--panel_of_normals", panel_of_normals)]
    extra = ["##molecules=the reads <movie>/<zmw>/ccs/fwd and <movie>/<zmw>/ccs/rev of one contig are the two strands of one "
             "molecule when each name has exactly one primary alignment there; a record is a substitution that both reads of "
             "at least one molecule show away from their trimmed ends, at --min_bq, with no more than --max_mismatch_count "
             "other mismatches in either read's window, both reads passing call's read filters",
             "##pile=DP, AD, VAF and the genotype count every read of the pile, as `himut sites` does: the two reads of a "
             "molecule are two reads, so AD x,2 with DS=1 is one molecule"]
    extra += ['##INFO=<ID={},Number={},Type={},Description="{}">'.format(*i) for i in _DUPLEX_INFOS]
    return _vcf_header("himut double-strand single base substitutions", extra, _DUPLEX_FILTERS,
                       dict(min_bq=min_bq, min_gq=min_gq, md_threshold=md_threshold), _DUPLEX_FORMATS, tname2tsize,
                       _run_command("duplex", bam_file, ref_file, region, region_list, opts, cs_from_ref), version, sample)


def duplex_lines(chrom, recs):
    """The data lines of the double-strand records of one contig (DUPLEX_RECORD_DTYPE) in _body_line's format: BQ = the alt
    quality sum over the alt count, DP = A+T+G+C+del, AD = ref,alt, VAF = alt / DP over every read of the pile; DS, SS and
    UNP in INFO and behind VAF in the sample column.  Germline (is_germ_gt explains the allele) is a FILTER value here, as
    it is a status of `himut sites`."""
    from ._ffi import SITE_STATUS_NAMES
    out = []
    for r in recs:
        ref, alt = chr(r["ref"]), chr(r["alt"])
        c = [int(x) for x in r["counts"]]
        depth = c[0] + c[1] + c[2] + c[3] + c[5]
        n_ref, n_alt = c[_ALLELE_IDX[ref]], c[_ALLELE_IDX[alt]]
        bq = int(r["alt_bqsum"]) / float(n_alt) if n_alt else 0.0
        ds, ss, unp = int(r["n_ds"]), int(r["n_ss"]), int(r["n_alt_unpaired"])
        sample = "./.:{}:{:0.1f}:{}:{},{}:{:.2f}:{}:{}:{}".format(int(r["gq"]), bq, depth, n_ref, n_alt, n_alt / float(depth) if depth else 0.0,
                                                                  ds, ss, unp)
        out.append("{}\t{}\t.\t{}\t{}\t.\t{}\tDS={};SS={};UNP={}\tGT:GQ:BQ:DP:AD:VAF:DS:SS:UNP\t{}\n".format(
            chrom, int(r["tpos"]), ref, alt, SITE_STATUS_NAMES[int(r["status"])], ds, ss, unp, sample))
    return out
