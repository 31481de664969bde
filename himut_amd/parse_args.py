"""Command lines of ``himut call``, ``germline``, ``support``, ``bqcal``, ``callable``, ``intervals``, ``dbs``, ``sites``, ``indels``, ``sindels``, ``indelcal``, ``haplotag``, ``duplex``, ``normcounts``, ``phase``,
``sbs96``, ``sbs1536``, ``sbs384``, ``id83``, ``dbs78``, ``fit``, ``burden`` and ``tricount`` (reference: src/himut/parse_args.py:37-692): same flag names, types and defaults,
plus ``--devices`` for the GPUs to use.  ``germline``, ``support``, ``bqcal``, ``callable``, ``intervals``, ``dbs``, ``sites``, ``indels``,
``sindels``, ``indelcal``, ``haplotag``, ``duplex``, ``sbs384``, ``id83``, ``dbs78`` and ``fit`` have no counterpart in the reference."""
import argparse
import sys


CS_FROM_REF_HELP = ("derive the cs text from CIGAR, SEQ and --ref during the BAM ingest: for BAM files without cs:Z tags "
                    "(pbmm2 output, archived HiFi BAMs); cs tags that are present are ignored")


def _add_sweep_flags(n, sbs_required, sbs_help, output_help):
    """The flags `normcounts` and `callable` share: same names, types and defaults."""
    n.add_argument("-i", "--bam", type=str, required=True,
                   help="minimap2 (parameters: -ax map-hifi --cs=short) aligned BAM file")
    n.add_argument("--ref", type=str, required=True, help="reference FASTA file")
    n.add_argument("--sbs", type=str, required=sbs_required, help=sbs_help)
    n.add_argument("--vcf", type=str, required=False, help="VCF file with germline mutations")
    n.add_argument("--phased_vcf", type=str, required=False, help="phased germline VCF file")
    n.add_argument("--common_snps", type=str, required=False, help="common SNPs VCF file")
    n.add_argument("--panel_of_normals", type=str, required=False, help="panel of normal VCF file")
    n.add_argument("--region", type=str, required=False, help="target chromosome")
    n.add_argument("--region_list", type=str, required=False, help="list of target chromosomes, one per line")
    n.add_argument("--min_qv", type=int, default=30, help="minimum read accuracy score")
    n.add_argument("--min_mapq", type=int, default=60, help="minimum mapping quality score")
    n.add_argument("--min_sequence_identity", type=float, default=0.99, help="minimum sequence identity")
    n.add_argument("--min_gq", type=int, default=20, help="minimum germline genotype quality score")
    n.add_argument("--min_bq", type=int, default=93, help="minimum base quality score")
    n.add_argument("--min_ref_count", type=int, default=3, help="minimum reference allele depth")
    n.add_argument("--min_alt_count", type=int, default=1, help="minimum alternative allele depth")
    n.add_argument("--min_hap_count", type=int, default=3, help="minimum h0 and h1 haplotype count")
    n.add_argument("--min_trim", type=float, default=0.01, help="proportion of the read ends to ignore")
    n.add_argument("--mismatch_window", type=int, default=20, help="mismatch window size")
    n.add_argument("--max_mismatch_count", type=int, default=0, help="maximum mismatches within the window")
    n.add_argument("--somatic_snv_prior", type=float, default=1 / (10 ** 6), help="somatic SNV prior")
    n.add_argument("--germline_snv_prior", type=float, default=1 / (10 ** 3), help="germline SNV prior")
    n.add_argument("--germline_indel_prior", type=float, default=1 / (10 ** 4), help="germline indel prior")
    n.add_argument("-t", "--threads", type=int, default=1, help="kept for the command line record; GPUs do the work")
    n.add_argument("--phase", required=False, action="store_true", help="use phased reads only")
    n.add_argument("--non_human_sample", required=False, action="store_true", help="human (default) or non-human sample")
    n.add_argument("--reference_sample", required=False, action="store_true", help="reads from the reference sample")
    n.add_argument("-o", "--output", type=str, required=True, help=output_help)
    n.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (contigs are spread over them)")
    n.add_argument("--cs_from_ref", required=False, action="store_true", help=CS_FROM_REF_HELP)


def build_parser(program_version):
    parser = argparse.ArgumentParser(
        prog="himut",
        description="himut identifies high-confidence single molecule somatic single-base substitutions from "
                    "PacBio CCS reads (MI355X build of the `call` path)")
    parser.add_argument("-v", "--version", action="version", version="%(prog)s {}".format(program_version))
    sub = parser.add_subparsers(dest="sub", metavar="")
    p = sub.add_parser("call", help="detects somatic mutations from circular consensus sequence (CCS) reads",
                       formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("-i", "--bam", type=str, required=True,
                   help="minimap2 (parameters: -ax map-hifi --cs=short) aligned BAM file")
    p.add_argument("--ref", type=str, required=False, help="reference genome FASTA file")
    p.add_argument("--vcf", type=str, required=False, help="VCF file with germline mutations")
    p.add_argument("--phased_vcf", type=str, required=False, help="phased germline VCF file")
    p.add_argument("--common_snps", type=str, required=False, help="common SNPs VCF file")
    p.add_argument("--panel_of_normals", type=str, required=False, help="panel of normal VCF file")
    p.add_argument("--region", type=str, required=False, help="target chromosome")
    p.add_argument("--region_list", type=str, required=False, help="list of target chromosomes, one per line")
    p.add_argument("--min_qv", type=int, default=30, help="minimum read accuracy score")
    p.add_argument("--min_mapq", type=int, default=60, help="minimum mapping quality score")
    p.add_argument("--min_sequence_identity", type=float, default=0.99, help="minimum sequence identity")
    p.add_argument("--min_gq", type=int, default=20, help="minimum germline genotype quality score")
    p.add_argument("--min_bq", type=int, default=93, help="minimum base quality score")
    p.add_argument("--min_ref_count", type=int, default=3, help="minimum reference allele depth")
    p.add_argument("--min_alt_count", type=int, default=1, help="minimum alternative allele depth")
    p.add_argument("--min_hap_count", type=int, default=3, help="minimum h0 and h1 haplotype count")
    p.add_argument("--min_trim", type=float, default=0.01, help="proportion of the read ends to ignore")
    p.add_argument("--max_mismatch_count", type=int, default=0, help="maximum mismatches within the window")
    p.add_argument("--mismatch_window_size", type=int, default=20, help="mismatch window size")
    p.add_argument("--somatic_snv_prior", type=float, default=1 / (10 ** 6), help="somatic SNV prior")
    p.add_argument("--germline_snv_prior", type=float, default=1 / (10 ** 3), help="germline SNV prior")
    p.add_argument("--germline_indel_prior", type=float, default=1 / (10 ** 4), help="germline indel prior")
    p.add_argument("-t", "--threads", type=int, default=1, help="kept for the header; GPUs do the work")
    p.add_argument("--phase", required=False, action="store_true", help="phase somatic mutations")
    p.add_argument("--non_human_sample", required=False, action="store_true", help="human (default) or non-human sample")
    p.add_argument("--reference_sample", required=False, action="store_true", help="reads from the reference sample")
    p.add_argument("--create_panel_of_normal", required=False, action="store_true",
                   help="call substitutions with relaxed parameters for panel of normal preparation")
    p.add_argument("-o", "--output", type=str, required=True, help="VCF file to write the substitutions")
    p.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (contigs are spread over them)")
    p.add_argument("--cs_from_ref", required=False, action="store_true", help=CS_FROM_REF_HELP)
    # himut germline (no counterpart in the reference: the germline VCF its phase / call --phase / --non_human_sample read)
    g = sub.add_parser("germline", help="calls germline SNVs (het, hom-alt, het-alt) from the CCS read pile",
                       formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    g.add_argument("-i", "--bam", type=str, required=True,
                   help="minimap2 (parameters: -ax map-hifi --cs=short) aligned BAM file")
    g.add_argument("--ref", type=str, required=False, help="reference genome FASTA file (for --cs_from_ref)")
    g.add_argument("--region", type=str, required=False, help="target chromosome")
    g.add_argument("--region_list", type=str, required=False, help="list of target chromosomes, one per line")
    g.add_argument("--min_mapq", type=int, default=0, help="minimum mapping quality score of a pile read")
    g.add_argument("--min_gq", type=int, default=20, help="minimum germline genotype quality score")
    g.add_argument("--min_bq", type=int, default=20, help="base quality score an alternative allele needs in one read")
    g.add_argument("--min_ref_count", type=int, default=2, help="minimum reference allele depth of a heterozygous site")
    g.add_argument("--min_alt_count", type=int, default=2, help="minimum alternative allele depth")
    g.add_argument("--germline_snv_prior", type=float, default=1 / (10 ** 3), help="germline SNV prior")
    g.add_argument("-t", "--threads", type=int, default=1, help="kept for the header; GPUs do the work")
    g.add_argument("-o", "--output", type=str, required=True, help="VCF file to write the germline SNVs")
    g.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (contigs are spread over them)")
    g.add_argument("--cs_from_ref", required=False, action="store_true", help=CS_FROM_REF_HELP)
    # himut support (no counterpart in the reference: its authors' scripts/sbs2ccs.py and sbs_qpos_distribution.py)
    u = sub.add_parser("support", help="lists the reads that carry each called substitution, one line per (site, read)",
                       description="One tab-separated line per called substitution and read that carries it: the read's name, "
                                   "strand (flag 0x10), mapping quality, length, the substitution's offset in the read "
                                   "(qpos, leading soft clip included, counted in the orientation the BAM stores: from the "
                                   "left end of SEQ whichever strand the read maps to), its base quality, the read's mean "
                                   "quality and its substitution, indel and mismatch-window counts.",
                       formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    u.add_argument("-i", "--bam", type=str, required=True,
                   help="minimap2 (parameters: -ax map-hifi --cs=short) aligned BAM file")
    u.add_argument("--sbs", type=str, required=True, help="himut VCF file (.vcf or .vcf.bgz) to read the substitutions from")
    u.add_argument("--all_filters", required=False, action="store_true", help="every data line of --sbs, not its PASS lines only")
    u.add_argument("--region", type=str, required=False, help="target chromosome")
    u.add_argument("--region_list", type=str, required=False, help="list of target chromosomes, one per line")
    u.add_argument("--min_mapq", type=int, default=0, help="minimum mapping quality score of a read")
    u.add_argument("--mismatch_window_size", type=int, default=20, help="mismatch window size")
    u.add_argument("--ref", type=str, required=False, help="reference genome FASTA file (for --cs_from_ref)")
    u.add_argument("--cs_from_ref", required=False, action="store_true", help=CS_FROM_REF_HELP)
    u.add_argument("-t", "--threads", type=int, default=1, help="BGZF inflate threads; the GPU finds the reads")
    u.add_argument("-o", "--output", type=str, required=True, help="TSV file to write the (site, read) lines; qpos counts "
                                                                    "in the orientation the BAM stores")
    u.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (contigs are spread over them)")
    # himut bqcal (no counterpart in the reference package: its authors' scripts/ccs2bq_calculation.py, whose flags these are)
    q = sub.add_parser("bqcal", help="tabulates the empirical base quality of every reported base quality",
                       description="One tab-separated line per reported base quality: the pile bases of that quality that "
                                   "disagree with a confidently called germline genotype (mismatch), those that agree "
                                   "(match), and pq = -10 log10(mismatch / match).  Where pq falls below the reported "
                                   "quality, --min_bq of `himut call` belongs above it.",
                       formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    q.add_argument("-i", "--bam", type=str, required=True,
                   help="minimap2 (parameters: -ax map-hifi --cs=short) aligned BAM file")
    q.add_argument("--ref", type=str, required=True, help="reference genome FASTA file")
    q.add_argument("--region", type=str, required=False, help="target chromosome")
    q.add_argument("--region_list", type=str, required=False, help="list of target chromosomes, one per line")
    q.add_argument("--min_mapq", type=int, default=0, help="minimum mapping quality score of a pile read")
    q.add_argument("--min_gq", type=int, default=20, help="minimum germline genotype quality score")
    q.add_argument("--germline_snv_prior", type=float, default=1 / (10 ** 3), help="germline SNV prior")
    q.add_argument("-t", "--threads", type=int, default=1, help="BGZF inflate threads; the GPU sweeps the positions")
    q.add_argument("-o", "--output", type=str, required=True, help="TSV file to write: bq, mismatch, match, pq")
    q.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (contigs are spread over them)")
    q.add_argument("--cs_from_ref", required=False, action="store_true", help=CS_FROM_REF_HELP)
    # himut dbs (no counterpart in the reference: cslib.cs2mut's tdbs_lst branch is never reached from `call`): call's
    # thresholds under call's names; no --phase
    d = sub.add_parser("dbs", help="detects somatic doublet base substitutions (CC>TT and the like) from the CCS read pile",
                       formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    d.add_argument("-i", "--bam", type=str, required=True,
                   help="minimap2 (parameters: -ax map-hifi --cs=short) aligned BAM file")
    d.add_argument("--ref", type=str, required=False, help="reference genome FASTA file (for --cs_from_ref)")
    d.add_argument("--common_snps", type=str, required=False, help="common SNPs VCF file")
    d.add_argument("--panel_of_normals", type=str, required=False, help="panel of normal VCF file")
    d.add_argument("--region", type=str, required=False, help="target chromosome")
    d.add_argument("--region_list", type=str, required=False, help="list of target chromosomes, one per line")
    d.add_argument("--min_qv", type=int, default=30, help="minimum read accuracy score")
    d.add_argument("--min_mapq", type=int, default=60, help="minimum mapping quality score")
    d.add_argument("--min_sequence_identity", type=float, default=0.99, help="minimum sequence identity")
    d.add_argument("--min_gq", type=int, default=20, help="minimum germline genotype quality score")
    d.add_argument("--min_bq", type=int, default=93, help="minimum base quality score")
    d.add_argument("--min_ref_count", type=int, default=3, help="minimum number of reads with both reference bases")
    d.add_argument("--min_alt_count", type=int, default=1, help="minimum number of reads with both alternative bases")
    d.add_argument("--min_trim", type=float, default=0.01, help="proportion of the read ends to ignore")
    d.add_argument("--max_mismatch_count", type=int, default=0, help="maximum mismatches within the window, the doublet aside")
    d.add_argument("--mismatch_window_size", type=int, default=20, help="mismatch window size")
    d.add_argument("--germline_snv_prior", type=float, default=1 / (10 ** 3), help="germline SNV prior")
    d.add_argument("-t", "--threads", type=int, default=1, help="kept for the header; GPUs do the work")
    d.add_argument("-o", "--output", type=str, required=True, help="VCF file to write the doublet base substitutions")
    d.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (contigs are spread over them)")
    d.add_argument("--cs_from_ref", required=False, action="store_true", help=CS_FROM_REF_HELP)
    # himut sites (no counterpart in the reference: its authors' pysam scripts): the thresholds of call's cascade under
    # call's names; no read filter shapes a pile, so none of call's read-filter flags
    s = sub.add_parser("sites", help="genotypes the substitutions of a himut VCF in another BAM: matched normal, another tissue",
                       description="One tab-separated line per substitution of --sbs: what this BAM's pile shows at the "
                                   "position -- the status `call`'s filters would give the substitution here (or Germline, "
                                   "or NoCoverage), the germline genotype and its quality, the depth, the reads per allele, "
                                   "the alt allele's mean base quality, its reads at or above --min_bq and --min_mapq, and "
                                   "the VAF.  --unseen writes the lines of --sbs this BAM does not show: the matched-normal "
                                   "subtraction.",
                       formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    s.add_argument("-i", "--bam", type=str, required=True,
                   help="minimap2 (parameters: -ax map-hifi --cs=short) aligned BAM file of the sample to look the sites up in")
    s.add_argument("--sbs", type=str, required=True, help="himut VCF file (.vcf or .vcf.bgz) to read the substitutions from")
    s.add_argument("--all_filters", required=False, action="store_true", help="every data line of --sbs, not its PASS lines only")
    s.add_argument("--common_snps", type=str, required=False, help="common SNPs VCF file")
    s.add_argument("--panel_of_normals", type=str, required=False, help="panel of normal VCF file")
    s.add_argument("--region", type=str, required=False, help="target chromosome")
    s.add_argument("--region_list", type=str, required=False, help="list of target chromosomes, one per line")
    s.add_argument("--min_mapq", type=int, default=60, help="mapping quality score an alt read needs to count in alt_mq")
    s.add_argument("--min_gq", type=int, default=20, help="minimum germline genotype quality score")
    s.add_argument("--min_bq", type=int, default=93, help="minimum base quality score")
    s.add_argument("--min_ref_count", type=int, default=3, help="minimum reference allele depth")
    s.add_argument("--min_alt_count", type=int, default=1, help="minimum alternative allele depth")
    s.add_argument("--germline_snv_prior", type=float, default=1 / (10 ** 3), help="germline SNV prior")
    s.add_argument("--unseen", type=str, required=False,
                   help="VCF file to write the lines of --sbs whose substitutions have no alt read and depth >= --min_depth here")
    s.add_argument("--min_depth", type=int, default=10, help="depth a site needs in this BAM to count as unseen (--unseen)")
    s.add_argument("--ref", type=str, required=False, help="reference genome FASTA file (for --cs_from_ref)")
    s.add_argument("--cs_from_ref", required=False, action="store_true", help=CS_FROM_REF_HELP)
    s.add_argument("-t", "--threads", type=int, default=1, help="BGZF inflate threads; the GPU genotypes the sites")
    s.add_argument("-o", "--output", type=str, required=True, help="TSV file to write, one line per site")
    s.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (contigs are spread over them)")
    # himut indels (no counterpart in the reference, where an indel only vetoes a site and --germline_indel_prior is never read)
    x = sub.add_parser("indels", help="calls germline short insertions and deletions from the CCS reads",
                       formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    x.add_argument("-i", "--bam", type=str, required=True,
                   help="minimap2 (parameters: -ax map-hifi --cs=short) aligned BAM file")
    x.add_argument("--ref", type=str, required=True, help="reference genome FASTA file")
    x.add_argument("--region", type=str, required=False, help="target chromosome")
    x.add_argument("--region_list", type=str, required=False, help="list of target chromosomes, one per line")
    x.add_argument("--min_mapq", type=int, default=0, help="minimum mapping quality score of a pile read")
    x.add_argument("--min_gq", type=int, default=20, help="minimum germline genotype quality score")
    x.add_argument("--min_ref_count", type=int, default=2, help="minimum number of other reads at a heterozygous allele")
    x.add_argument("--min_alt_count", type=int, default=2, help="minimum number of reads that carry the allele")
    x.add_argument("--germline_indel_prior", type=float, default=1 / (10 ** 4), help="germline indel prior")
    x.add_argument("--indel_error", type=float, default=0.01,
                   help="per-read probability of an indel error: one constant, a definition; --error_table puts this "
                        "BAM's own measurement (`himut indelcal`) in its place")
    x.add_argument("--error_table", type=str, required=False,
                   help="TSV file of `himut indelcal`: the per-read error of an allele in a homopolymer run comes from "
                        "the row of the run's letter and length")
    x.add_argument("--min_spans", type=int, default=1000,
                   help="spanning reads a row of --error_table needs; a row with fewer keeps --indel_error")
    x.add_argument("--max_indel_len", type=int, default=50, choices=range(1, 65), metavar="[1-64]",
                   help="longest insertion or deletion to call")
    x.add_argument("--cs_from_ref", required=False, action="store_true", help=CS_FROM_REF_HELP)
    x.add_argument("-t", "--threads", type=int, default=1, help="BGZF inflate threads; the GPU calls the indels")
    x.add_argument("-o", "--output", type=str, required=True, help="VCF file to write the indels")
    x.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (contigs are spread over them)")
    # himut sindels (no counterpart in the reference): the third COSMIC class beside `call` (SBS) and `dbs`
    si = sub.add_parser("sindels", help="lists somatic insertion and deletion candidates carried by single CCS reads",
                        description="Candidates under stated rules, not calls: HiFi indel error outside repeats is orders of "
                                    "magnitude above a somatic indel rate, and inside homopolymers it is higher still.  A "
                                    "candidate is an allele that a read passing `call`'s read filters shows away from its "
                                    "trimmed ends, with no other mismatch in the window and every base of its footprint at "
                                    "--min_bq, in a pile that genotypes hom-ref.  FILTER: IndelSite (another indel at the "
                                    "anchor), Repeat (the allele lengthens or shortens a homopolymer run longer than "
                                    "--max_run; repeats of longer units are not recognised), LowGQ, LowDepth, HighDepth, "
                                    "PASS.  himut_sindels.log keeps the counters needed to subtract an expected error load "
                                    "(`himut indelcal` gives the rate).  --max_run, --indel_error and the footprint rule are "
                                    "definitions chosen here.",
                        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    si.add_argument("-i", "--bam", type=str, required=True,
                    help="minimap2 (parameters: -ax map-hifi --cs=short) aligned BAM file")
    si.add_argument("--ref", type=str, required=True, help="reference genome FASTA file")
    si.add_argument("--region", type=str, required=False, help="target chromosome")
    si.add_argument("--region_list", type=str, required=False, help="list of target chromosomes, one per line")
    si.add_argument("--min_qv", type=int, default=30, help="minimum read accuracy score")
    si.add_argument("--min_mapq", type=int, default=60, help="minimum mapping quality score")
    si.add_argument("--min_sequence_identity", type=float, default=0.99, help="minimum sequence identity")
    si.add_argument("--min_gq", type=int, default=20, help="minimum genotype quality score of the hom-ref pile")
    si.add_argument("--min_bq", type=int, default=93, help="minimum base quality score of every base of the footprint")
    si.add_argument("--min_ref_count", type=int, default=3, help="minimum number of reads without an indel at the anchor")
    si.add_argument("--min_alt_count", type=int, default=1, help="minimum number of reads that carry the allele")
    si.add_argument("--min_trim", type=float, default=0.01, help="proportion of the read ends to ignore")
    si.add_argument("--max_mismatch_count", type=int, default=0, help="maximum other mismatches within the window")
    si.add_argument("--mismatch_window_size", type=int, default=20, help="mismatch window size")
    si.add_argument("--germline_indel_prior", type=float, default=1 / (10 ** 4), help="germline indel prior")
    si.add_argument("--indel_error", type=float, default=0.01,
                    help="per-read probability of an indel error: one constant, a definition; --error_table puts this "
                         "BAM's own measurement (`himut indelcal`) in its place")
    si.add_argument("--error_table", type=str, required=False,
                    help="TSV file of `himut indelcal`: the per-read error of an allele in a homopolymer run comes from "
                         "the row of the run's letter and length")
    si.add_argument("--min_spans", type=int, default=1000,
                    help="spanning reads a row of --error_table needs; a row with fewer keeps --indel_error")
    si.add_argument("--max_indel_len", type=int, default=50, choices=range(1, 65), metavar="[1-64]",
                    help="longest insertion or deletion to list")
    si.add_argument("--max_run", type=int, default=2,
                    help="longest homopolymer run in which a deletion, or an insertion of the run's letter, is not "
                         "filtered as Repeat: a definition chosen here")
    si.add_argument("--cs_from_ref", required=False, action="store_true", help=CS_FROM_REF_HELP)
    si.add_argument("-t", "--threads", type=int, default=1, help="BGZF inflate threads; the GPU does the work")
    si.add_argument("-o", "--output", type=str, required=True, help="VCF file to write the candidates")
    si.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (contigs are spread over them)")
    # himut indelcal (no counterpart in the reference): what --indel_error of `indels` is worth on this BAM
    ic = sub.add_parser("indelcal", help="tabulates the empirical indel error of the reads per homopolymer run of the reference",
                        description="One tab-separated line per class of homopolymer run (its letter, its length; lengths "
                                    "32 to 64 share the last row): the runs of the regions, the runs set aside because "
                                    "their anchor looks like a germline variant (excluded), the pile reads that span the "
                                    "others (spans), and the indel events those reads show in them -- deletions and "
                                    "insertions of the run's own letter by length 1, 2, 3 and more, and anything else -- "
                                    "with del_rate and ins_rate, events per spanning read.  `himut indels --error_table` "
                                    "reads the file.",
                        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ic.add_argument("-i", "--bam", type=str, required=True,
                    help="minimap2 (parameters: -ax map-hifi --cs=short) aligned BAM file")
    ic.add_argument("--ref", type=str, required=True, help="reference genome FASTA file")
    ic.add_argument("--region", type=str, required=False, help="target chromosome")
    ic.add_argument("--region_list", type=str, required=False, help="list of target chromosomes, one per line")
    ic.add_argument("--min_mapq", type=int, default=0, help="minimum mapping quality score of a pile read")
    ic.add_argument("--min_alt_count", type=int, default=2,
                    help="reads an allele needs for its anchor to count as a variant (with --germline_vaf)")
    ic.add_argument("--germline_vaf", type=float, default=0.25,
                    help="allele fraction from which an anchor counts as a variant and its run is set aside")
    ic.add_argument("--max_indel_len", type=int, default=50, choices=range(1, 65), metavar="[1-64]",
                    help="longest insertion or deletion to count")
    ic.add_argument("--cs_from_ref", required=False, action="store_true", help=CS_FROM_REF_HELP)
    ic.add_argument("-t", "--threads", type=int, default=1, help="BGZF inflate threads; the GPU counts")
    ic.add_argument("-o", "--output", type=str, required=True, help="TSV file to write, one line per class of run")
    ic.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (contigs are spread over them)")
    # himut normcounts (reference: parse_args.py:502-692)
    n = sub.add_parser("normcounts", help="normalises SBS96 mutation counts based on genome and read trinucleotide "
                                          "context counts", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    _add_sweep_flags(n, True, "himut VCF file to read somatic single base substitutions",
                     "file to write the normalised SBS96 counts")
    # himut callable (no counterpart in the reference): the flags of normcounts, --sbs optional
    cl = sub.add_parser("callable", help="writes where the caller could have called: the normcounts verdict of every position "
                                         "as BED runs",
                        description="One BED line per stretch of equal state: chrom, start, end (0-based, half open), STATE, "
                                    "bases (the callable read bases over the stretch).  STATE is the row of norm.log the "
                                    "positions add to: CALLABLE, NO_BASE, UNPHASED, HET, HETALT, HOMALT, INDEL, HIGH_DEPTH, "
                                    "ALLELE_BALANCE, LOW_GQ, PON, COMMON_SNP, or NON_ACGT for a reference letter that is no "
                                    "upper-case A/C/G/T.  The positions swept are those of the chunks `normcounts` sweeps "
                                    "(with --phase: the phase blocks).  Stretches of equal state that abut across a chunk "
                                    "boundary are written as one line; chunks that overlap or leave gaps are written as they "
                                    "come, and a position outside every chunk appears in no line.",
                        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    _add_sweep_flags(cl, False, "himut VCF file of `himut call`: the depth threshold and the read length limits come from its "
                                "header; without it they are computed from the BAM as `himut call` computes them",
                     "BED file to write")
    cl.add_argument("--callable_only", required=False, action="store_true", help="write the CALLABLE lines only")
    cl.add_argument("--summary", type=str, required=False, help="file to write one line per contig and state: positions, bases")
    # himut intervals (no counterpart in the reference): the flags of callable, the intervals, the side files
    iv = sub.add_parser("intervals", help="writes callable counts and the mutation burden per BED interval or fixed-width bin",
                        description="One tab-separated line per interval: chrom, start, end (0-based, half open), name, "
                                    "length, the swept positions inside it (entries), its CALLABLE positions and their "
                                    "callable read bases, and with --sbs the substitutions inside it, those that fall "
                                    "where nothing is callable, the rate per callable base and the burden per cell.  "
                                    "The run in front is `himut callable`: every flag of it means here what it means there.",
                        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    _add_sweep_flags(iv, False, "himut VCF file of `himut call`: its header gives the thresholds, as in `callable`, and its "
                                "PASS single base substitutions are counted per interval",
                     "TSV file to write, one line per interval")
    which = iv.add_mutually_exclusive_group(required=True)
    which.add_argument("--bed", type=str, help="BED file: chrom, start, end and optionally a name, tab-separated")
    which.add_argument("--bin_size", type=int, help="width of the bins to cut every swept contig into")
    iv.add_argument("--tri", type=str, required=False,
                    help="file to write 33 lines per interval: the trinucleotide class, all_tri, ref_tri, ccs_tri, sbs")
    iv.add_argument("--states", type=str, required=False, help="file to write one line per interval and state: positions, bases")
    iv.add_argument("--genes", type=str, required=False,
                    help="genes for --strands: BED with at least six columns, or GFF3 / GTF (.gff, .gff3, .gtf)")
    iv.add_argument("--feature", type=str, default="gene", help="the GFF3 / GTF records --genes takes (third column)")
    iv.add_argument("--strands", type=str, required=False,
                    help="file to write, per contig, transcription-strand category (T, U, B, N as in `himut sbs384`) and "
                         "trinucleotide: the CALLABLE positions, their callable bases and, with --sbs, the substitutions; "
                         "needs --genes")
    # himut haplotag (no counterpart in the reference: its authors' scripts/sbs2hap.py)
    ht = sub.add_parser("haplotag", help="assigns each read to a haplotype of the phased hetSNPs it spans, one line per read",
                        description="One tab-separated line per read: the phase set (PS) and haplotype (HP, 1 or 2) the read's "
                                    "bases at the phased hetSNPs vote for, a status (Assigned, NotInPile, NoSnp, NoVote, "
                                    "LowSupport, Conflict) and the votes behind it.  --snps adds one line per phased hetSNP: "
                                    "what the reads show there, and how many assigned reads agree or disagree with its "
                                    "phase.  The counters go to himut_haplotag.log.",
                        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ht.add_argument("-i", "--bam", type=str, required=True,
                    help="minimap2 (parameters: -ax map-hifi --cs=short) aligned BAM file")
    ht.add_argument("--phased_vcf", type=str, required=True, help="phased germline VCF file (himut phase)")
    ht.add_argument("-o", "--output", type=str, required=True, help="TSV file to write, one line per read")
    ht.add_argument("--snps", type=str, required=False, help="TSV file to write, one line per phased hetSNP")
    ht.add_argument("--min_mapq", type=int, default=0, help="minimum mapping quality score of a pile read")
    ht.add_argument("--min_bq", type=int, default=20, help="minimum base quality score of a base that votes")
    ht.add_argument("--min_snps", type=int, default=1, help="votes a read needs in its phase set to be assigned")
    ht.add_argument("--min_agree", type=float, default=0.8,
                    help="share of a read's votes its haplotype needs, 0.501 to 1 (compared in permille)")
    ht.add_argument("--region", type=str, required=False, help="target chromosome")
    ht.add_argument("--region_list", type=str, required=False, help="list of target chromosomes, one per line")
    ht.add_argument("--ref", type=str, required=False, help="reference genome FASTA file (for --cs_from_ref)")
    ht.add_argument("--cs_from_ref", required=False, action="store_true", help=CS_FROM_REF_HELP)
    ht.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (contigs are spread over them)")
    ht.add_argument("-t", "--threads", type=int, default=1, help="BGZF inflate threads; the GPU assigns the reads")
    # himut duplex (no counterpart in the reference, which takes every alignment as a molecule of its own): call's thresholds
    # under call's names; no --phase
    dx = sub.add_parser("duplex", help="detects substitutions that both strands of one molecule show (`ccs --by-strand` reads)",
                        description="For a BAM of `ccs --by-strand` reads (<movie>/<zmw>/ccs/fwd and .../rev, one per DNA "
                                    "strand): one VCF line per substitution that both reads of at least one molecule show, "
                                    "each read under call's read and event rules, with the verdict call's filters give the "
                                    "position.  DS counts the molecules that show it on both strands, SS the reads that show "
                                    "it against a mate with the reference base, UNP the alt reads outside any such pair.  The "
                                    "pile counts every read, so a molecule adds two to DP and AD.  --ss writes the spectrum "
                                    "of the single-strand events and the number of positions both strands cover well enough "
                                    "to have shown a mutation.  The counters go to himut_duplex.log.",
                        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    dx.add_argument("-i", "--bam", type=str, required=True,
                    help="minimap2 (parameters: -ax map-hifi --cs=short) aligned BAM file of by-strand reads")
    dx.add_argument("-o", "--output", type=str, required=True, help="VCF file to write the double-strand substitutions")
    dx.add_argument("--ss", type=str, required=False,
                    help="TSV file to write the twelve single-strand classes and the double-strand denominator")
    dx.add_argument("--ref", type=str, required=False, help="reference genome FASTA file (for --cs_from_ref)")
    dx.add_argument("--common_snps", type=str, required=False, help="common SNPs VCF file")
    dx.add_argument("--panel_of_normals", type=str, required=False, help="panel of normal VCF file")
    dx.add_argument("--region", type=str, required=False, help="target chromosome")
    dx.add_argument("--region_list", type=str, required=False, help="list of target chromosomes, one per line")
    dx.add_argument("--min_qv", type=int, default=30, help="minimum read accuracy score")
    dx.add_argument("--min_mapq", type=int, default=60, help="minimum mapping quality score")
    dx.add_argument("--min_sequence_identity", type=float, default=0.99, help="minimum sequence identity")
    dx.add_argument("--min_gq", type=int, default=20, help="minimum germline genotype quality score")
    dx.add_argument("--min_bq", type=int, default=93, help="minimum base quality score, on either strand")
    dx.add_argument("--min_ref_count", type=int, default=3, help="minimum reference allele depth")
    dx.add_argument("--min_alt_count", type=int, default=1, help="minimum alternative allele depth")
    dx.add_argument("--min_trim", type=float, default=0.01, help="proportion of the read ends to ignore, on either strand")
    dx.add_argument("--max_mismatch_count", type=int, default=0, help="maximum mismatches within the window, on either strand")
    dx.add_argument("--mismatch_window_size", type=int, default=20, help="mismatch window size")
    dx.add_argument("--germline_snv_prior", type=float, default=1 / (10 ** 3), help="germline SNV prior")
    dx.add_argument("-t", "--threads", type=int, default=1, help="BGZF inflate threads; the GPU does the work")
    dx.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (contigs are spread over them)")
    dx.add_argument("--cs_from_ref", required=False, action="store_true", help=CS_FROM_REF_HELP)
    # himut phase (reference: parse_args.py:343-415)
    h = sub.add_parser("phase", help="returns phased hetsnps", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    h.add_argument("-i", "--bam", type=str, required=True,
                   help="minimap2 (parameters: -ax map-hifi --cs=short) aligned BAM file")
    h.add_argument("--vcf", type=str, required=True, help="deepvariant VCF file with germline mutations")
    h.add_argument("--region", type=str, required=False, help="target chromosome")
    h.add_argument("--region_list", type=str, required=False, help="list of target chromosomes separated by new line")
    h.add_argument("--min_bq", type=int, default=20, help="minimum base quality score threshold")
    h.add_argument("--min_mapq", type=int, default=20, help="minimum mapping quality score")
    h.add_argument("--min_p_value", type=float, default=0.0001, help="maximum binomial p-value of a phase consistent edge")
    h.add_argument("--min_phase_proportion", type=float, default=0.2, help="minimum proportion of phase consistent edges")
    h.add_argument("-t", "--threads", type=int, default=1, help="BGZF inflate threads; the GPU counts the edges")
    h.add_argument("-o", "--output", type=str, required=True, help="VCF file to write phased hetsnps")
    h.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (the first one is used)")
    h.add_argument("--ref", type=str, required=False, help="reference FASTA file (for --cs_from_ref)")
    h.add_argument("--cs_from_ref", required=False, action="store_true", help=CS_FROM_REF_HELP)
    # himut sbs96 / sbs1536 (reference: parse_args.py:267-342): the TSV only, the plots need plotnine
    for name, what in (("sbs96", "SBS96"), ("sbs1536", "SBS1536")):
        m = sub.add_parser(name, help="returns {} counts".format(what), formatter_class=argparse.ArgumentDefaultsHelpFormatter)
        m.add_argument("-i", "--input", type=str, required=True, help="himut VCF file to read somatic single base substitutions")
        m.add_argument("--ref", type=str, required=True, help="reference FASTA file")
        m.add_argument("--region", type=str, required=False, help="target chromosome")
        m.add_argument("--region_list", type=str, required=False, help="list of target chromosomes separated by new line")
        m.add_argument("-o", "--output", type=str, required=True, help="file to return {} counts (.tsv suffix)".format(what))
        m.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (the first one is used)")
    # himut sbs384 (no counterpart in the reference): the transcription-strand spectrum and its opportunity counts
    s384 = sub.add_parser("sbs384", help="returns SBS384 counts: the SBS96 classes split by transcription strand",
                          description="The substitutions `sbs96` counts, split by where they lie relative to the genes of "
                                      "--genes.  These definitions are this package's (DESIGN.md section 8 row 18).  A gene "
                                      "is a stranded interval; every position of a contig lies in no gene, in genes on +, "
                                      "in genes on -, or in both.  The category of a substitution depends on that and on "
                                      "whether its REF is a purine, that is, is read on the other strand by `sbs96`: no "
                                      "gene N; both B; a + gene gives U for a pyrimidine REF and T for a purine REF; a - gene "
                                      "gives T for a pyrimidine REF and U for a purine REF.  T means the pyrimidine of the "
                                      "pair lies on the transcribed (template) strand, SigProfiler's convention.  The "
                                      "classes are labelled T:A[C>A]A, in the order T, U, B, N with the 96 in `sbs96`'s "
                                      "order inside each.  --opp counts the reference's trinucleotides the same way, by the "
                                      "centre letter: a trinucleotide counts when its three letters are upper-case ACGT.  "
                                      "What `sbs96` raises for is counted in himut_sbs384.log, with the other counters.",
                          formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    s384.add_argument("-i", "--input", type=str, required=True, help="himut VCF file to read somatic single base substitutions")
    s384.add_argument("--ref", type=str, required=True, help="reference FASTA file")
    s384.add_argument("--genes", type=str, required=True,
                      help="genes: BED with at least six columns (chrom, start, end, name, score, strand), or GFF3 / GTF "
                           "(.gff, .gff3, .gtf); records without a + or - strand are counted and skipped")
    s384.add_argument("--feature", type=str, default="gene", help="the GFF3 / GTF records --genes takes (third column)")
    s384.add_argument("--region", type=str, required=False, help="target chromosome")
    s384.add_argument("--region_list", type=str, required=False, help="list of target chromosomes separated by new line")
    s384.add_argument("-o", "--output", type=str, required=True, help="file to return SBS384 counts (.tsv suffix)")
    s384.add_argument("--sbs192", type=str, required=False, help="file to write the T and U blocks alone (SBS192)")
    s384.add_argument("--opp", type=str, required=False,
                      help="file to write category, trinucleotide and its count in the reference, summed over the contigs")
    s384.add_argument("--classes", type=str, required=False,
                      help="TSV file to write one line per classified substitution: chrom, pos, ref, alt, sbs384")
    s384.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (the first one is used)")
    # himut id83 / dbs78 (no counterpart in the reference): the spectra of the VCFs `indels`, `sindels` and `dbs` write
    definition = ("The classes are COSMIC's, labelled in SigProfiler's form; the rules that put an allele into a class are "
                  "this package's definition of the COSMIC scheme (DESIGN.md section 8 row 17).  ")
    i83 = sub.add_parser("id83", help="returns ID83 counts of an indel VCF (`himut indels`, `himut sindels`)",
                         description=definition + "An indel's repeat is the periodic extent of the allele on both sides of "
                                     "where the VCF places it, compared without case: the class does not depend on the "
                                     "placement inside the repeat.  1-base alleles are classed by letter and homopolymer "
                                     "length, longer ones by the copies of the unit, deletions with an extent shorter than "
                                     "their length as microhomology.  Every ALT allele of a line is taken on its own; "
                                     "alleles of equal length, complex alleles, alleles longer than 64 and deletions whose "
                                     "REF disagrees with --ref are counted in himut_id83.log and skipped.",
                         formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    i83.add_argument("-i", "--input", type=str, required=True, help="VCF file (.vcf or .vcf.bgz) to read the indels from")
    i83.add_argument("--ref", type=str, required=True, help="reference FASTA file")
    i83.add_argument("--region", type=str, required=False, help="target chromosome")
    i83.add_argument("--region_list", type=str, required=False, help="list of target chromosomes separated by new line")
    i83.add_argument("--all_filters", required=False, action="store_true", help="every data line of --input, not its PASS lines only")
    i83.add_argument("--classes", type=str, required=False,
                     help="TSV file to write one line per classified allele: chrom, pos, ref, alt, id83")
    i83.add_argument("-o", "--output", type=str, required=True, help="file to return ID83 counts (.tsv suffix)")
    i83.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (the first one is used)")
    d78 = sub.add_parser("dbs78", help="returns DBS78 counts of a doublet VCF (`himut dbs`)",
                         description=definition + "The lines with a two-letter REF and a two-letter ALT are taken; a doublet "
                                     "whose reference pair is not one of the ten of the scheme is read on the other strand.  "
                                     "The counters go to himut_dbs78.log.",
                         formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    d78.add_argument("-i", "--input", type=str, required=True, help="VCF file (.vcf or .vcf.bgz) to read the doublets from")
    d78.add_argument("--region", type=str, required=False, help="target chromosome")
    d78.add_argument("--region_list", type=str, required=False, help="list of target chromosomes separated by new line")
    d78.add_argument("--all_filters", required=False, action="store_true", help="every data line of --input, not its PASS lines only")
    d78.add_argument("-o", "--output", type=str, required=True, help="file to return DBS78 counts (.tsv suffix)")
    d78.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (the first one is used)")
    # himut fit (no counterpart in the reference): signature exposures of a spectrum, with bootstrap intervals
    ft = sub.add_parser("fit", help="returns the exposures of given signatures in a spectrum, with bootstrap intervals",
                        description="Which of the given signatures explain a spectrum, and how much of each.  The definition "
                                    "is this package's (DESIGN.md section 8 row 20).  Inputs: integer counts m[c], c < C, "
                                    "N their sum, and a non-negative matrix S[c][k], k < K, whose columns each sum to 1.  "
                                    "Fit: multiplicative EM for the Poisson / multinomial mixture, --iters iterations, no "
                                    "early stop.  Start e[k] = N / K.  Step 1, for every c: r[c] = sum over k of S[c][k] * "
                                    "e[k], summed sequentially in ascending k from 0.0, and q[c] = 0.0 if m[c] == 0 or "
                                    "r[c] == 0.0, else m[c] / r[c].  Step 2, for every k: g = sum over c of S[c][k] * q[c], "
                                    "summed sequentially in ascending c from 0.0, and e[k] = e[k] * g.  All arithmetic is "
                                    "fp64, one multiply and one add per term, nothing contracted.  Bootstrap: replicate 0 is "
                                    "the spectrum; replicate b (1 <= b <= B) draws N mutations, draw i (0 <= i < N) taking "
                                    "z = seed + 0x9E3779B97F4A7C15 * (1 + b * 2^32 + i), z = (z ^ (z >> 30)) * "
                                    "0xBF58476D1CE4E5B9, z = (z ^ (z >> 27)) * 0x94D049BB133111EB, z ^= z >> 31 (all mod "
                                    "2^64), j = ((z >> 32) * N) >> 32, and landing in the smallest c whose inclusive prefix "
                                    "sum of m exceeds j; each replicate is fitted as above.  Limits: 1 <= C <= 1536, 1 <= K "
                                    "<= 96, N < 2^31, B <= 100000, 1 <= iters <= 100000.  "
                                    "The spectrum is any table this package writes (sbs96, sbs1536, sbs384 and its --sbs192, "
                                    "id83, dbs78, normcounts): its header is the first line with a field named counts, its "
                                    "labels are the column just before, lines before the header are skipped.  The "
                                    "signatures are a tab-separated matrix in COSMIC's layout: labels in the first column, a "
                                    "signature per further column; rows are matched to the spectrum by label, in any order, "
                                    "and a label missing on either side is an error.  Channels in which every selected "
                                    "signature is 0 are set aside and their counts reported as unexplained.  With --opp the "
                                    "matrix becomes S[c][k] * w[c], renormalised per column, so the fit runs in the sample's "
                                    "space; exposure is then the mutations observed and exposure_genome = exposure / (sum "
                                    "over c of S[c][k] * w[c]), rescaled so that the column sums to N: what the genome-wide "
                                    "spectrum would attribute.  Without --opp the two are equal.  With --bootstrap above 0 "
                                    "lo, median and hi are the 2.5 / 50 / 97.5 percentiles of the replicates' exposures and "
                                    "presence the share of replicates whose fraction is at least --min_fraction.  The "
                                    "counters go to himut_fit.log.",
                        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ft.add_argument("-i", "--input", type=str, required=True, help="spectrum: a table of sbs96, sbs1536, sbs384, id83, dbs78 or normcounts")
    ft.add_argument("--signatures", type=str, required=True, help="signature matrix (.tsv): labels, then a column per signature")
    ft.add_argument("--select", type=str, required=False, help="comma separated signature names to fit, in this order; without it every column")
    ft.add_argument("--opp", type=str, required=False,
                    help="opportunities: a table of label and weight, or the word normcounts to take 1 / (ref_tri_ratio * "
                         "ref_ccs_tri_ratio) from the normcounts table given as --input")
    ft.add_argument("--bootstrap", type=int, default=1000, help="bootstrap replicates (0: the point fit alone)")
    ft.add_argument("--seed", type=int, default=1, help="seed of the bootstrap's draws (taken mod 2^64)")
    ft.add_argument("--iters", type=int, default=1000, help="EM iterations")
    ft.add_argument("--min_fraction", type=float, default=0.05, help="the fraction from which a replicate counts a signature as present")
    ft.add_argument("--recon", type=str, required=False, help="file to write label, counts and reconstructed")
    ft.add_argument("--boot", type=str, required=False, help="file to write the replicate x signature matrix of exposures")
    ft.add_argument("-o", "--output", type=str, required=True, help="file to return the exposures (.tsv suffix)")
    ft.add_argument("--device", type=int, default=0, help="GPU id")
    # himut burden (reference: parse_args.py:416-462)
    b = sub.add_parser("burden", help="calculates mutation burden per cell", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    b.add_argument("-i", "--input", type=str, required=True, help="normalised SBS96 counts")
    b.add_argument("--ref", type=str, required=False, help="reference FASTA file")
    b.add_argument("--tri", type=str, required=False, help="reference trinucleotide sequence context")
    b.add_argument("--region_list", type=str, required=False,
                   help="list of autosomes and sex chromosomes separated by new line")
    b.add_argument("-t", "--threads", type=int, default=1, required=False, help="kept for the reference's command line; the GPU counts")
    b.add_argument("-o", "--output", type=str, required=True, help="file to return mutation burden per cell")
    b.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (the first one is used)")
    # himut tricount (reference: parse_args.py:463-501)
    t = sub.add_parser("tricount", help="calculates and returns reference trinucletide context counts",
                       formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    t.add_argument("-i", "--ref", type=str, required=True, help="reference FASTA file")
    t.add_argument("--region", type=str, required=False, help="target chromosome")
    t.add_argument("--region_list", type=str, required=False, help="list of target chromosomes separated by new line")
    t.add_argument("-t", "--threads", type=int, default=1, required=False, help="kept for the reference's command line; the GPU counts")
    t.add_argument("-o", "--output", type=str, required=True, help="file to return reference trinucleotide counts")
    t.add_argument("--devices", type=str, default="0", help="comma separated GPU ids (the first one is used)")
    return parser


def parse_args(program_version, arguments=None):
    parser = build_parser(program_version)
    if arguments is None:
        arguments = sys.argv[1:]
    if len(arguments) == 0:          # parse_args.py:693-695: help and exit 0
        parser.print_help()
        parser.exit()
    options = parser.parse_args(arguments)
    if getattr(options, "cs_from_ref", False) and not options.ref:
        parser.error("--cs_from_ref needs --ref: the cs text is derived from the reference bases under each alignment")
    if options.sub in ("id83", "dbs78", "sbs384") and options.region is not None and options.region_list is not None:
        parser.error("--region or --region_list, not both")
    if options.sub == "intervals" and (options.genes is None) != (options.strands is None):
        parser.error("--genes and --strands go together")
    if options.sub == "haplotag":
        from .haplotag import agree_permille
        try:
            options.min_agree_permille = agree_permille(options.min_agree)
        except ValueError as e:
            parser.error(str(e))
        if options.min_snps < 1:
            parser.error("--min_snps must be at least 1")
    return parser, options
