"""Hand-built alignments for the indelcal run's contract: one case per rule and per shape at
which a kernel can go wrong.  A case is (name, batch, regions, contig string, parameters, expect(table, log as a dict));
the CPU tests run the model on them and check what each rule says, the GPU tests compare the run with the model and check
the same statements.  The contigs are random strings without a stretch of three equal letters, so that the planted runs
are the only ones of their classes."""
import numpy as np

from tests import indelcal_model as K
from tests.indels_cases import batch, read

N = 3000


def contig(seed, n=N, plant=()):
    """A random ACGT string in which no letter stands three times in a row, with the given (position, string) planted."""
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        c = "ACGT"[rs.randint(4)]
        if len(out) >= 2 and out[-1] == out[-2] == c:
            continue
        out.append(c)
    s = "".join(out)
    for pos, t in plant:
        s = s[:pos] + t + s[pos + len(t):]
    return s[:n]


def run_of(b, n, left=None, right=None):
    """A run of n letters b between two other letters."""
    other = [x for x in "CGAT" if x != b.upper()]
    return (left or other[0]) + b * n + (right or other[1])


def cell(table, b, n, column):
    return int(table[K.run_class(b, n)][K.col(column)])


def _cases():
    out = []

    def case(name, recs, ref, expect, regions=None, **kw):
        out.append((name, batch(recs, len(ref)), regions or [(0, len(ref))], ref, kw,
                    lambda t, l, expect=expect: expect(t, dict(zip(K.LOG, l)))))

    def over(ref, n, start=100, length=None, **event):
        return [read(ref, start, length or len(ref) - 200, **event) for _ in range(n)]

    # ---- block boundaries.  A run across 256; G at 511 (a run of one starting at 255 + 256) with T * 12 from 512, its
    # anchor 511 the last position of a block
    ref = contig(1, plant=[(250, run_of("A", 10)), (510, "CG" + "T" * 12 + "C")])

    def blocks(t, l):
        assert cell(t, "A", 10, "runs") == 1 and cell(t, "A", 10, "spans") == 5
        assert cell(t, "T", 12, "runs") == 1 and cell(t, "T", 12, "spans") == 5
        assert l["runs_long"] == 0 and l["events"] == 0 and l["runs_excluded"] == 0
    case("block_straddle_and_edges", over(ref, 5), ref, blocks)
    ref = contig(2, plant=[(254, "C" + "T" * 9 + "G"), (767, "CA" + "G" * 11 + "T")])

    def starts(t, l):                                            # T * 9 from 255; A at 768 = 3 * 256, G * 11 from 769
        assert cell(t, "T", 9, "runs") == 1 and cell(t, "T", 9, "spans") == 4
        assert cell(t, "G", 11, "runs") == 1 and cell(t, "G", 11, "spans") == 4
    case("block_run_starts_255_256", over(ref, 4), ref, starts)

    # ---- run lengths around the last bin and the long limit
    ref = contig(3, plant=[(100 + 200 * k, run_of("A", n)) for k, n in enumerate((31, 32, 33, 64, 65))])
    recs = over(ref, 7) + [read(ref, 100, N - 200, dels={720: 1}), read(ref, 100, N - 200, dels={930: 1})]

    def lengths(t, l):
        assert cell(t, "A", 31, "runs") == 1 and cell(t, "A", 32, "runs") == 3 and l["runs_long"] == 1
        assert cell(t, "A", 31, "spans") == 9 and cell(t, "A", 32, "spans") == 27
        assert cell(t, "A", 32, "del1") == 1 and l["num_offrun"] == 1 and l["events_counted"] == 1    # the 65-run is long
    case("run_lengths_31_to_65", recs, ref, lengths)

    # ---- reference edges
    ref = contig(4, plant=[(0, "G" + "T" * 7 + "C")])            # a run at position 1
    ref = ref[:N - 8] + "C" + "G" * 7                             # a stretch that reaches the end: no run
    recs = [read(ref, 0, N) for _ in range(3)] + [read(ref, 0, N, dels={N - 3: 1})]

    def edges(t, l):
        assert cell(t, "T", 7, "runs") == 1 and cell(t, "T", 7, "spans") == 4
        assert cell(t, "G", 7, "runs") == 0 and l["num_offrun"] == 1 and l["events"] == 1
    case("edge_run_at_1_and_stretch_to_end", recs, ref, edges)
    ref = contig(5, plant=[(0, "A" * 8 + "C")])                   # a stretch from 0: no run; the shift stops at position 1
    recs = [read(ref, 0, N - 100) for _ in range(3)] + [read(ref, 0, N - 100, dels={4: 1})]

    def from_zero(t, l):
        assert cell(t, "A", 8, "runs") == 0 and l["num_offrun"] == 1 and l["events_counted"] == 0
    case("edge_stretch_from_0", recs, ref, from_zero)

    # ---- letters: lower case, N as a flank, N inside a stretch
    ref = contig(6, plant=[(300, "c" + "a" * 4 + "A" * 4 + "g"), (600, "N" + "G" * 9 + "N"), (900, "C" + "T" * 11 + "N" + "T" * 13 + "G")])
    recs = over(ref, 5) + [read(ref, 100, N - 200, dels={303: 1}), read(ref, 100, N - 200, ins={915: "T"})]

    def letters(t, l):
        assert cell(t, "A", 8, "runs") == 1 and cell(t, "G", 9, "runs") == 1
        assert cell(t, "T", 11, "runs") == 1 and cell(t, "T", 13, "runs") == 1 and cell(t, "T", 24, "runs") == 0
        assert cell(t, "A", 8, "del1") == 1 and cell(t, "T", 13, "ins1") == 1 and cell(t, "G", 9, "spans") == 7
    case("letters_lower_case_and_n", recs, ref, letters)

    # ---- spans.  C at 1000, A * 10 from 1001, G at 1011: a = 1000, s + n = 1011
    ref = contig(7, plant=[(1000, run_of("A", 10))])
    recs = [read(ref, 1000, 300), read(ref, 1001, 300),           # tstart == a spans, a + 1 does not
            read(ref, 700, 311), read(ref, 700, 312),             # tend == s + n does not, s + n + 1 does
            read(ref, 1000, 12),                                  # wholly inside the run and its flanks
            read(ref, 1003, 5), read(ref, 995, 10)]               # shorter than the run

    def spans(t, l):
        assert cell(t, "A", 10, "runs") == 1 and cell(t, "A", 10, "spans") == 3
    case("span_boundaries", recs, ref, spans)
    recs = over(ref, 4) + [read(ref, 100, N - 200, flag=0x100), read(ref, 100, N - 200, mapq=5),
                           read(ref, 100, N - 200, flag=0x100, dels={1004: 1}), read(ref, 100, N - 200, mapq=5, dels={1004: 1})]

    def filters(t, l):
        assert cell(t, "A", 10, "spans") == 4 and l["events"] == 0
    case("span_read_filters", recs, ref, filters, min_mapq=20)

    # ---- regions
    def once(t, l):
        assert cell(t, "A", 10, "runs") == 1 and cell(t, "A", 10, "spans") == 4 and cell(t, "A", 10, "del1") == 1
    one = over(ref, 3) + [read(ref, 100, N - 200, dels={1005: 1})]
    case("region_overlap_and_touch", one, ref, once, regions=[(900, 1000), (1000, 1100), (950, 1050), (1101, 1200)])
    case("region_first_position", one, ref, once, regions=[(1000, 1400)])
    case("region_last_position", one, ref, once, regions=[(600, 1000)])

    def outside(t, l):
        assert cell(t, "A", 10, "runs") == 0 and l["events"] == 0 and l["runs"] > 0
    case("region_anchor_outside", one, ref, outside, regions=[(0, 999), (1001, N)])

    # ---- more window reads than the sweep holds in LDS at a time (256): 300 short reads over the run, 290 beside it
    recs = [read(ref, 990, 40) for _ in range(300)] + [read(ref, 1001 + k % 3, 40) for k in range(290)] + [read(ref, 990, 40, dels={1003: 1})]

    def crowded(t, l):
        assert cell(t, "A", 10, "spans") == 301 and cell(t, "A", 10, "del1") == 1
    case("window_over_the_stage", recs, ref, crowded)

    # ---- the variant rule
    ref = contig(8, plant=[(1000, run_of("A", 10)), (2000, run_of("T", 12))])
    recs = over(ref, 2) + over(ref, 2, dels={1004: 1}) + [read(ref, 1500, 1000) for _ in range(3)] + [read(ref, 1500, 1000, dels={2005: 1}) for _ in range(3)]

    def alt_count(t, l):                                          # min_alt_count 3: two carriers are one short, three are there
        assert cell(t, "A", 10, "excluded") == 0 and cell(t, "A", 10, "del1") == 2 and cell(t, "A", 10, "spans") == 4
        assert cell(t, "T", 12, "excluded") == 1 and cell(t, "T", 12, "spans") == 0 and cell(t, "T", 12, "del1") == 0
        assert l["variant_anchors"] == 1 and l["anchors"] == 2 and l["events_variant"] == 3
    case("variant_min_alt_count", recs, ref, alt_count, min_alt_count=3, vaf_permille=250)
    recs = over(ref, 6, length=1200) + over(ref, 2, length=1200, dels={1004: 1}) + [read(ref, 1500, 1000) for _ in range(7)] + \
           [read(ref, 1500, 1000, dels={2005: 1}) for _ in range(2)]

    def vaf(t, l):                                                # 2 of 8 is 250 permille, 2 of 9 one read short of it
        assert cell(t, "A", 10, "excluded") == 1 and cell(t, "T", 12, "excluded") == 0
        assert cell(t, "T", 12, "del1") == 2 and cell(t, "T", 12, "spans") == 9 and l["events_variant"] == 2
    case("variant_vaf", recs, ref, vaf, min_alt_count=2, vaf_permille=250)

    # ---- event columns.  C at 1000, A * 4 from 1001, G at 1005
    ref = contig(9, plant=[(1000, run_of("A", 4))])
    recs = over(ref, 6) + [read(ref, 100, N - 200, dels={1001: 4}), read(ref, 100, N - 200, dels={1001: 5}),
                           read(ref, 100, N - 200, ins={1003: "AA"}), read(ref, 100, N - 200, ins={1001: "GA"}),
                           read(ref, 100, N - 200, ins={1001: "A"}, dels={1001: 1}), read(ref, 100, N - 200, dels={1002: 2})]

    def columns(t, l):
        row = [cell(t, "A", 4, k) for k in K.COLUMNS]
        assert row == [1, 0, 12, 1, 1, 1, 1, 1, 0, 2], row        # +a-a in one read: two events against one span
        assert l["events"] == l["events_counted"] == 7 and l["anchors"] == 1
    case("event_columns", recs, ref, columns)

    # ---- event rules: the shift stops at the read's start inside the run; the read ends inside the run
    ref = contig(10, plant=[(1000, run_of("A", 10))])
    recs = over(ref, 5) + [read(ref, 1004, 300, dels={1007: 1}), read(ref, 700, 308, dels={1003: 1})]

    def rules(t, l):
        assert l["num_offrun"] == 1 and l["num_partial"] == 1 and l["events_counted"] == 0 and l["events"] == 2
        assert cell(t, "A", 10, "spans") == 5
    case("event_offrun_and_partial", recs, ref, rules)

    def nothing(t, l):
        assert l["events"] == 0 and l["spans"] == 0 and l["runs"] > 1000
    case("shape_no_reads_over_the_regions", [read(ref, 0, 50)], ref, nothing, regions=[(100, N)])
    return out


CASES = _cases()
