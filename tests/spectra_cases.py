"""Hand-built strings and indel alleles for the ID83 contract, each with the label it must get
written down from the construction, not computed by a classifier: CASES is a list of (name, seq, anchor, kind, L, inserted
bases, label).  A deletion removes seq[anchor+1 .. anchor+L]; an insertion goes between seq[anchor] and seq[anchor+1]."""
from tests.spectra_model import NBASE, RANGE

CASES = []


def case(name, seq, a, kind, L, ins, label):
    assert kind in ("del", "ins") and (kind == "del" or len(ins) == L)
    CASES.append((name, seq, a, kind, L, ins, label))


# ---- 1-base alleles in homopolymer runs of 1..7 (6 and 7: the 6+ cap), both letters, both strands.
# flank + run + flank with flanks of other letters; the deletion is the run's first base, the insertion goes in front of it
for letter, rep, left, right in (("A", "T", "GC", "CG"), ("T", "T", "GC", "CG"), ("C", "C", "AT", "GA"), ("G", "C", "AT", "CA")):
    for k in range(1, 8):
        seq = left + letter * k + right
        case("del1_{}_run{}".format(letter, k), seq, 1, "del", 1, "", "1:Del:{}:{}".format(rep, min(k - 1, 5)))
    for k in range(0, 8):
        seq = left + letter * k + right
        case("ins1_{}_run{}".format(letter, k), seq, 1, "ins", 1, letter, "1:Ins:{}:{}".format(rep, min(k, 5)))

# ---- repeats of a unit of 2, 3, 4, 5, 6 and 64 letters: k copies between flanks that continue nothing
U64 = "ACGGTCAG" * 7 + "ACGGTCAC"
UNITS = {2: "AC", 3: "ACG", 4: "ACGG", 5: "ACGTC", 6: "ACGGTC", 64: U64}
for L, unit in UNITS.items():
    size = min(L, 5)
    copies = range(1, 8) if L <= 5 else (5, 6, 7)          # a deletion leaves k - 1: 4, 5 and 6 copies left at k = 5, 6, 7
    for k in copies:
        seq = "TT" + unit * k + "TT"
        case("del{}_copies{}".format(L, k), seq, 1, "del", L, "", "{}:Del:R:{}".format(size, min(k - 1, 5)))
    for k in (range(0, 8) if L <= 5 else (4, 5, 6)):
        seq = "TT" + unit * k + "TT"
        case("ins{}_copies{}".format(L, k), seq, 1, "ins", L, unit, "{}:Ins:R:{}".format(size, min(k, 5)))

# ---- microhomology: the deleted stretch, then its first h letters again, then a letter that ends the match
case("mh2_1", "TT" + "AC" + "A" + "GG", 1, "del", 2, "", "2:Del:M:1")
case("mh3_1", "TT" + "ACG" + "A" + "TT", 1, "del", 3, "", "3:Del:M:1")
case("mh3_2", "TT" + "ACG" + "AC" + "TT", 1, "del", 3, "", "3:Del:M:2")
case("mh3_3_is_a_repeat", "TT" + "ACG" + "ACG" + "TT", 1, "del", 3, "", "3:Del:R:1")       # m = L: one copy left
case("mh4_1", "TT" + "ACGG" + "A" + "TT", 1, "del", 4, "", "4:Del:M:1")
case("mh4_2", "TT" + "ACGG" + "AC" + "TT", 1, "del", 4, "", "4:Del:M:2")
case("mh4_3", "TT" + "ACGG" + "ACG" + "TT", 1, "del", 4, "", "4:Del:M:3")
case("mh4_4_is_a_repeat", "TT" + "ACGG" + "ACGG" + "TT", 1, "del", 4, "", "4:Del:R:1")
case("mh5_1", "GG" + "ACGTC" + "A" + "TT", 1, "del", 5, "", "5:Del:M:1")
case("mh5_2", "GG" + "ACGTC" + "AC" + "TT", 1, "del", 5, "", "5:Del:M:2")
case("mh5_3", "GG" + "ACGTC" + "ACG" + "GG", 1, "del", 5, "", "5:Del:M:3")
case("mh5_4", "GG" + "ACGTC" + "ACGT" + "TT", 1, "del", 5, "", "5:Del:M:4")
case("mh5_5_is_a_repeat", "GG" + "ACGTC" + "ACGTC" + "TT", 1, "del", 5, "", "5:Del:R:1")
case("mh6_5", "TT" + "ACGGTC" + "ACGGT" + "AA", 1, "del", 6, "", "5:Del:M:5")
case("mh6_6_is_a_repeat", "TT" + "ACGGTC" + "ACGGTC" + "AA", 1, "del", 6, "", "5:Del:R:1")
case("mh7_5", "TT" + "ACGGTCA" + "ACGGT" + "GG", 1, "del", 7, "", "5:Del:M:5")
case("mh7_6_cap", "TT" + "ACGGTCA" + "ACGGTC" + "GG", 1, "del", 7, "", "5:Del:M:5")       # microhomology 6 reports as 5
# microhomology on the left of the placed allele only: TT AC [GAC] T -- deleting GAC, the AC in front repeats its end
case("mh3_left", "TT" + "AC" + "GAC" + "TT", 3, "del", 3, "", "3:Del:M:2")
# a 64-letter deletion followed by its first 63 letters: microhomology 63, one letter short of a repeat
case("mh64_63", "TT" + U64 + U64[:63] + "TT", 1, "del", 64, "", "5:Del:M:5")

# ---- one event at every placement inside its repeat: GG ACACAC TT
REP = "GG" + "ACACAC" + "TT"
for a in (1, 2, 3, 4, 5):
    case("placed_del2_at{}".format(a), REP, a, "del", 2, "", "2:Del:R:2")
for a in (1, 2, 3, 4, 5, 6, 7):
    case("placed_ins2_at{}".format(a), REP, a, "ins", 2, "AC" if a % 2 else "CA", "2:Ins:R:3")
# a 3-letter unit: TT ACGACGACG TT, the insertion's bases rotated with the anchor
REP3 = "TT" + "ACG" * 3 + "TT"
for a, ins in ((1, "ACG"), (2, "CGA"), (3, "GAC"), (4, "ACG"), (5, "CGA"), (10, "ACG")):
    case("placed_ins3_at{}".format(a), REP3, a, "ins", 3, ins, "3:Ins:R:3")
for a in range(1, 8):
    case("placed_del3_at{}".format(a), REP3, a, "del", 3, "", "3:Del:R:2")
# a 1-base deletion in the middle of its run: the letter on both sides
for a in (1, 2, 3, 4, 5):
    case("placed_del1_at{}".format(a), "GT" + "AAAAA" + "CG", a, "del", 1, "", "1:Del:T:4")
for a in (1, 2, 3, 4, 5, 6):
    case("placed_ins1_at{}".format(a), "GT" + "AAAAA" + "CG", a, "ins", 1, "A", "1:Ins:T:5")

# ---- the ends of the string
case("anchor0_del", "GAAC", 0, "del", 1, "", "1:Del:T:1")
case("anchor0_ins", "GAAC", 0, "ins", 1, "A", "1:Ins:T:2")
case("anchor0_ins_of_the_first_letter", "GAAC", 0, "ins", 1, "G", "1:Ins:C:1")
case("left_end_in_scan", "AAAC", 0, "del", 1, "", "1:Del:T:2")
case("left_end_in_scan_ins", "AAAC", 1, "ins", 1, "A", "1:Ins:T:3")
case("left_end_in_scan_unit", "ACACACG", 3, "del", 2, "", "2:Del:R:2")
case("del_ends_at_last_base", "GCAA", 2, "del", 1, "", "1:Del:T:1")
case("del2_ends_at_last_base", "GTACAC", 3, "del", 2, "", "2:Del:R:1")
case("del2_ends_at_last_base_partial_copy", "GCACAC", 3, "del", 2, "", "2:Del:R:1")      # m = 3: one copy and a half
case("ins_behind_last_base", "GCAA", 3, "ins", 1, "A", "1:Ins:T:2")
case("ins_behind_last_base_unit", "GCACAC", 5, "ins", 2, "AC", "2:Ins:R:2")
case("right_end_in_scan", "GCAAA", 1, "del", 1, "", "1:Del:T:2")
case("right_end_in_scan_ins", "GCAAA", 1, "ins", 1, "A", "1:Ins:T:3")
case("whole_string_is_the_run", "AAAAAAAA", 3, "del", 1, "", "1:Del:T:5")
case("range_del_negative", "GCAA", -1, "del", 1, "", RANGE)
case("range_del_last", "GCAA", 3, "del", 1, "", RANGE)
case("range_del_runs_out", "GCAA", 2, "del", 2, "", RANGE)
case("range_del_far", "GCAA", 1000, "del", 64, "", RANGE)
case("range_ins_negative", "GCAA", -1, "ins", 1, "A", RANGE)
case("range_ins_behind", "GCAA", 4, "ins", 1, "A", RANGE)

# ---- case: soft-masked stretches compare as their upper-case letters
case("lower_del", "gtaaaacg", 1, "del", 1, "", "1:Del:T:3")
case("mixed_del", "GTaAaACG", 3, "del", 1, "", "1:Del:T:3")
case("lower_ins", "gtaaaacg", 1, "ins", 1, "A", "1:Ins:T:4")
case("mixed_unit_del", "ttAcaCACtt", 1, "del", 2, "", "2:Del:R:2")
case("mixed_unit_ins", "ttAcaCACtt", 4, "ins", 2, "CA", "2:Ins:R:3")
case("lower_g_del", "atgggca", 2, "del", 1, "", "1:Del:C:2")

# ---- letters outside ACGT end a scan, and match nothing -- not even themselves
case("n_ends_scan", "GTAANAACG", 1, "del", 1, "", "1:Del:T:1")
case("r_ends_scan", "GTAARAACG", 1, "del", 1, "", "1:Del:T:1")
case("n_ends_scan_left", "GTAANAACG", 5, "del", 1, "", "1:Del:T:1")
case("n_ends_scan_ins", "GTAANAACG", 3, "ins", 1, "A", "1:Ins:T:2")
case("n_ends_scan_unit", "TTACACNACTT", 1, "del", 2, "", "2:Del:R:1")
case("n_in_both_copies", "TTACNACNTT", 1, "del", 3, "", NBASE)
case("n_between_copies", "TTACGNACGNTT", 1, "del", 3, "", "3:Del:R:0")          # ACG N ACG N: the N stops the scan at once
case("n_in_deleted_stretch", "GGANCTT", 1, "del", 3, "", NBASE)
case("n_is_the_deleted_base", "GGNTT", 1, "del", 1, "", NBASE)
case("lower_n_in_deleted_stretch", "GGAnCTT", 1, "del", 3, "", NBASE)
case("ins_next_to_n", "GGNTT", 1, "ins", 1, "G", "1:Ins:C:2")

# ---- a hand-written FASTA and VCF for the host parser and the two subcommands, with what they must write
C1 = "GTAAAAACGTTACACACTTGG"           # G0 T1 A2..A6 C7 G8 T9 T10 (AC)x3 at 11..16 T17 T18 G19 G20
C2 = "ttacgacgacgtt"                   # soft-masked: (acg)x3 at 2..10
FASTA_TEXT = ">c1 first\n" + C1[:8] + "\n" + C1[8:] + "\n>c2\n" + C2 + "\n"


def _line(chrom, pos, ref, alt, flt="PASS"):
    return "\t".join([chrom, str(pos), ".", ref, alt, "30", flt, ".", "GT:GQ", "0/1:30"]) + "\n"


VCF_TEXT = (
    "##fileformat=VCFv4.2\n"
    "##contig=<ID=c1,length=21>\n##contig=<ID=c2,length=13>\n##contig=<ID=c3,length=100>\n"
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n" +
    _line("c1", 1, "G", "G" + "A" * 65) +            # longer than 64
    _line("c1", 2, "TA", "T") +                      # one A of the run of five: 1:Del:T:4
    _line("c1", 2, "T", "TA,TC") +                   # multi-allelic: 1:Ins:T:5 and 1:Ins:C:0
    _line("c1", 8, "C", "G") +                       # an SNV
    _line("c1", 8, "CG", "TT") +                     # a doublet: CG>TT
    _line("c1", 8, "CG", "CT") +                     # a doublet with an unchanged base
    _line("c1", 9, "GT", "AC") +                     # a doublet read on the other strand: AC>GT
    _line("c1", 9, "GTT", "CT,GA") +                 # complex twice: first bases differ; neither allele of length 1
    _line("c1", 11, "TAC", "T", "LowGQ") +           # not PASS: one AC of three, 2:Del:R:2
    _line("c1", 13, "CAG", "C") +                    # REF disagrees with the FASTA (CAC)
    _line("c1", 15, "NN", "AC") +                    # a doublet with a letter outside ACGT
    _line("c1", 19, "TG", "CA", "LowBQ") +           # not PASS: TG>CA
    _line("c1", 20, "G", "GN") +                     # an inserted N
    _line("c2", 2, "T", "TACG") +                    # in front of three copies: 3:Ins:R:3
    _line("c2", 2, "TACG", "T") +                    # REF is the upper-cased string: 3:Del:R:2
    _line("c2", 14, "T", "TA") +                     # behind the string
    _line("c3", 5, "AT", "A"))                       # a contig the FASTA lacks

# {all_filters: (counts by label, the --classes lines, the log's cells per contig in ID83_LOG_ROWS order)}
ID83_EXPECT = {
    False: ({"1:Del:T:4": 1, "1:Ins:T:5": 1, "1:Ins:C:0": 1, "3:Ins:R:3": 1, "3:Del:R:2": 1},
            ["c1\t2\tTA\tT\t1:Del:T:4", "c1\t2\tT\tTA\t1:Ins:T:5", "c1\t2\tT\tTC\t1:Ins:C:0", "c2\t2\tT\tTACG\t3:Ins:R:3",
             "c2\t2\tTACG\tT\t3:Del:R:2"],
            {"c1": [13, 5, 2, 1, 1, 1, 0, 3], "c2": [3, 0, 0, 0, 0, 0, 1, 2]}),
    True: ({"1:Del:T:4": 1, "1:Ins:T:5": 1, "1:Ins:C:0": 1, "2:Del:R:2": 1, "3:Ins:R:3": 1, "3:Del:R:2": 1},
           ["c1\t2\tTA\tT\t1:Del:T:4", "c1\t2\tT\tTA\t1:Ins:T:5", "c1\t2\tT\tTC\t1:Ins:C:0", "c1\t11\tTAC\tT\t2:Del:R:2",
            "c2\t2\tT\tTACG\t3:Ins:R:3", "c2\t2\tTACG\tT\t3:Del:R:2"],
           {"c1": [15, 6, 2, 1, 1, 1, 0, 4], "c2": [3, 0, 0, 0, 0, 0, 1, 2]}),
}
ID83_ABSENT = {"c3": 1}
# {all_filters: (counts by label, the log's cells per contig: doublets, non-ACGT, unchanged, classified)}
DBS78_EXPECT = {
    False: ({"CG>TT": 1, "AC>GT": 1}, {"c1": [4, 1, 1, 2], "c2": [0, 0, 0, 0], "c3": [0, 0, 0, 0]}),
    True: ({"CG>TT": 1, "AC>GT": 1, "TG>CA": 1}, {"c1": [5, 1, 1, 3], "c2": [0, 0, 0, 0], "c3": [0, 0, 0, 0]}),
}
