#!/usr/bin/env python3
"""``python -m himut_amd call | germline | support | bqcal | callable | intervals | dbs | sites | indels | sindels | indelcal | haplotag | duplex | normcounts | phase | sbs96 | sbs1536 | sbs384 | id83 | dbs78 | fit | burden | tricount ...``
-- the `himut` entry points (reference: src/himut/__main__.py:15-188; sbs52 and the plots are left out;
``germline``, ``support``, ``bqcal``, ``callable``, ``intervals``, ``dbs``, ``sites``, ``indels``, ``sindels``, ``indelcal``, ``haplotag``, ``duplex``,
``id83``, ``dbs78`` and ``fit`` are this package's own; ``id83`` and ``dbs78`` class alleles by this package's definition of the
COSMIC scheme, ``fit`` gives signature exposures by this package's definition of the fit and its bootstrap)."""
__version__ = "1.0.4+mi355x"

import sys

from himut_amd.parse_args import parse_args


def main(arguments=None):
    parser, options = parse_args(__version__, arguments)
    devices = [int(d) for d in getattr(options, "devices", "").split(",") if d != ""]
    if options.sub == "call":
        from himut_amd import caller
        caller.call_somatic_substitutions(
            options.bam, options.ref, options.vcf, options.phased_vcf, options.common_snps, options.panel_of_normals,
            options.region, options.region_list, options.min_qv, options.min_mapq, options.min_sequence_identity,
            options.min_gq, options.min_bq, options.min_trim, options.max_mismatch_count, options.mismatch_window_size,
            options.min_ref_count, options.min_alt_count, options.min_hap_count, options.somatic_snv_prior,
            options.germline_snv_prior, options.germline_indel_prior, options.threads, options.phase,
            options.non_human_sample, options.reference_sample, options.create_panel_of_normal, __version__,
            options.output, devices=devices, cs_from_ref=options.cs_from_ref)
    elif options.sub == "germline":
        from himut_amd import germline
        germline.call_germline_snvs(
            options.bam, options.region, options.region_list, options.min_mapq, options.min_gq, options.min_bq,
            options.min_ref_count, options.min_alt_count, options.germline_snv_prior, options.threads, __version__,
            options.output, devices=devices, ref_file=options.ref, cs_from_ref=options.cs_from_ref)
    elif options.sub == "support":
        from himut_amd import support
        support.dump_support(
            options.bam, options.sbs, options.region, options.region_list, options.min_mapq, options.mismatch_window_size,
            options.all_filters, options.threads, options.output, devices=devices, ref_file=options.ref,
            cs_from_ref=options.cs_from_ref)
    elif options.sub == "bqcal":
        from himut_amd import bqcal
        bqcal.dump_empirical_bq(
            options.bam, options.ref, options.region, options.region_list, options.min_mapq, options.min_gq,
            options.germline_snv_prior, options.threads, options.output, devices=devices, cs_from_ref=options.cs_from_ref)
    elif options.sub == "callable":
        from himut_amd import callable as callable_
        callable_.dump_callable(
            options.bam, options.ref, options.sbs, options.vcf, options.phased_vcf, options.common_snps,
            options.panel_of_normals, options.region, options.region_list, options.min_qv, options.min_mapq,
            options.min_sequence_identity, options.min_gq, options.min_bq, options.min_trim, options.mismatch_window,
            options.max_mismatch_count, options.min_ref_count, options.min_alt_count, options.min_hap_count,
            options.somatic_snv_prior, options.germline_snv_prior, options.germline_indel_prior, options.threads,
            options.phase, options.non_human_sample, options.reference_sample, options.output,
            callable_only=options.callable_only, summary_file=options.summary, devices=devices,
            cs_from_ref=options.cs_from_ref)
    elif options.sub == "intervals":
        from himut_amd import intervals
        intervals.dump_intervals(
            options.bam, options.ref, options.bed, options.bin_size, options.sbs, options.vcf, options.phased_vcf,
            options.common_snps, options.panel_of_normals, options.region, options.region_list, options.min_qv,
            options.min_mapq, options.min_sequence_identity, options.min_gq, options.min_bq, options.min_trim,
            options.mismatch_window, options.max_mismatch_count, options.min_ref_count, options.min_alt_count,
            options.min_hap_count, options.somatic_snv_prior, options.germline_snv_prior, options.germline_indel_prior,
            options.threads, options.phase, options.non_human_sample, options.reference_sample, options.output,
            tri_file=options.tri, states_file=options.states, devices=devices, cs_from_ref=options.cs_from_ref,
            genes_file=options.genes, feature=options.feature, strands_file=options.strands)
    elif options.sub == "dbs":
        from himut_amd import dbs
        dbs.call_doublet_substitutions(
            options.bam, options.common_snps, options.panel_of_normals, options.region, options.region_list, options.min_qv,
            options.min_mapq, options.min_sequence_identity, options.min_gq, options.min_bq, options.min_trim,
            options.max_mismatch_count, options.mismatch_window_size, options.min_ref_count, options.min_alt_count,
            options.germline_snv_prior, options.threads, __version__, options.output, devices=devices, ref_file=options.ref,
            cs_from_ref=options.cs_from_ref)
    elif options.sub == "sites":
        from himut_amd import sites
        argv = sys.argv[1:] if arguments is None else list(arguments)
        sites.dump_sites(
            options.bam, options.sbs, options.common_snps, options.panel_of_normals, options.region, options.region_list,
            options.min_mapq, options.min_gq, options.min_bq, options.min_ref_count, options.min_alt_count,
            options.germline_snv_prior, options.all_filters, options.threads, options.output, devices=devices,
            ref_file=options.ref, cs_from_ref=options.cs_from_ref, unseen_file=options.unseen, min_depth=options.min_depth,
            command="himut " + " ".join(argv))
    elif options.sub == "indels":
        from himut_amd import indels
        indels.call_germline_indels(
            options.bam, options.ref, options.region, options.region_list, options.min_mapq, options.min_gq,
            options.min_ref_count, options.min_alt_count, options.germline_indel_prior, options.indel_error,
            options.max_indel_len, options.threads, __version__, options.output, devices=devices,
            cs_from_ref=options.cs_from_ref, error_table=options.error_table, min_spans=options.min_spans)
    elif options.sub == "sindels":
        from himut_amd import sindels
        sindels.call_somatic_indels(
            options.bam, options.ref, options.region, options.region_list, options.min_qv, options.min_mapq,
            options.min_sequence_identity, options.min_gq, options.min_bq, options.min_trim, options.mismatch_window_size,
            options.max_mismatch_count, options.min_ref_count, options.min_alt_count, options.germline_indel_prior,
            options.indel_error, options.max_indel_len, options.max_run, options.threads, __version__, options.output,
            devices=devices, cs_from_ref=options.cs_from_ref, error_table=options.error_table,
            min_spans=options.min_spans)
    elif options.sub == "indelcal":
        from himut_amd import indelcal
        indelcal.dump_indel_error(
            options.bam, options.ref, options.region, options.region_list, options.min_mapq, options.min_alt_count,
            options.germline_vaf, options.max_indel_len, options.threads, options.output, devices=devices,
            cs_from_ref=options.cs_from_ref)
    elif options.sub == "haplotag":
        from himut_amd import haplotag
        haplotag.dump_haplotags(
            options.bam, options.phased_vcf, options.region, options.region_list, options.min_mapq, options.min_bq,
            options.min_snps, options.min_agree_permille, options.threads, options.output, snps_file=options.snps,
            devices=devices, ref_file=options.ref, cs_from_ref=options.cs_from_ref)
    elif options.sub == "duplex":
        from himut_amd import duplex
        duplex.call_duplex_substitutions(
            options.bam, options.common_snps, options.panel_of_normals, options.region, options.region_list, options.min_qv,
            options.min_mapq, options.min_sequence_identity, options.min_gq, options.min_bq, options.min_trim,
            options.max_mismatch_count, options.mismatch_window_size, options.min_ref_count, options.min_alt_count,
            options.germline_snv_prior, options.threads, __version__, options.output, ss_file=options.ss, devices=devices,
            ref_file=options.ref, cs_from_ref=options.cs_from_ref)
    elif options.sub == "normcounts":
        from himut_amd import normcounts
        normcounts.get_normcounts(
            options.bam, options.ref, options.sbs, options.vcf, options.phased_vcf, options.common_snps,
            options.panel_of_normals, options.region, options.region_list, options.min_qv, options.min_mapq,
            options.min_sequence_identity, options.min_gq, options.min_bq, options.min_trim, options.mismatch_window,
            options.max_mismatch_count, options.min_ref_count, options.min_alt_count, options.min_hap_count,
            options.somatic_snv_prior, options.germline_snv_prior, options.germline_indel_prior, options.threads,
            options.phase, options.non_human_sample, options.reference_sample, options.output, devices=devices,
            cs_from_ref=options.cs_from_ref)
    elif options.sub == "phase":
        from himut_amd import phaselib
        phaselib.get_chrom_hblock(
            options.bam, options.vcf, options.region, options.region_list, options.min_bq, options.min_mapq,
            options.min_p_value, options.min_phase_proportion, options.threads, __version__, options.output,
            devices=devices, ref_file=options.ref, cs_from_ref=options.cs_from_ref)
    elif options.sub in ("sbs96", "sbs1536"):
        from himut_amd import mutlib
        if options.region is not None and options.region_list is not None:      # util.check_mutpatterns_input_exists
            print("Please provide input for --region or --region_list parameter and not for both parameters")
            print("One or more inputs and parameters are missing")
            print("Please provide the correct inputs and parameters")
            print("exiting himut")
            sys.exit(0)
        _sample, tname2tsize = mutlib.get_sample(options.input)
        dump = mutlib.dump_sbs96_counts if options.sub == "sbs96" else mutlib.dump_sbs1536_counts
        dump(options.input, options.ref, options.region, options.region_list, tname2tsize, options.output,
             device=devices[0])
    elif options.sub == "sbs384":
        from himut_amd import strands
        strands.dump_sbs384_counts(options.input, options.ref, options.genes, options.region, options.region_list,
                                   options.output, feature=options.feature, sbs192_file=options.sbs192, opp_file=options.opp,
                                   classes_file=options.classes, device=devices[0])
    elif options.sub == "id83":
        from himut_amd import spectra
        spectra.dump_id83_counts(options.input, options.ref, options.region, options.region_list, options.output,
                                 all_filters=options.all_filters, classes_file=options.classes, device=devices[0])
    elif options.sub == "dbs78":
        from himut_amd import spectra
        spectra.dump_dbs78_counts(options.input, options.region, options.region_list, options.output,
                                  all_filters=options.all_filters, device=devices[0])
    elif options.sub == "fit":
        from himut_amd import fit
        try:
            fit.dump_exposures(options.input, options.signatures, options.output, select=options.select, opp=options.opp,
                               n_boot=options.bootstrap, seed=options.seed, iters=options.iters,
                               min_fraction=options.min_fraction, recon_file=options.recon, boot_file=options.boot,
                               device=options.device)
        except fit.FitError as e:
            print("himut fit: {}".format(e), file=sys.stderr)
            sys.exit(1)
    elif options.sub == "burden":
        from himut_amd import mutlib
        from himut_amd.reflib import get_genome_tricounts_device
        mutlib.get_burden_per_cell(
            options.input, options.ref, options.tri, options.region_list, options.threads, options.output,
            tricounts=lambda path, chrom_lst: get_genome_tricounts_device(path, chrom_lst, devices[0]))
    elif options.sub == "tricount":
        from himut_amd import reflib
        reflib.get_ref_tricount(options.ref, options.region, options.region_list, options.threads, options.output,
                                device=devices[0])
    else:
        parser.print_help()


if __name__ == "__main__":
    main()
