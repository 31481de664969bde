"""The contig feed's assignment of contigs to devices (himut_amd/feed.py), without a device."""
from himut_amd import bamio, dist as hdist, feed
from himut_amd.readbatch import batch_from_records

SIZES = {"chr1": 900, "chr2": 600, "chr3": 400, "chr10": 300, "chr11": 300, "chrX": 100}


def _drivers_comprehension(sizes, devices):
    """What every driver spelled out itself before the feed."""
    return [(c, d) for d, contigs in zip(devices, hdist.lpt_assign(sizes, len(devices))) for c in contigs]


def test_share_over_devices_narrowed_and_empty(tmp_path):
    want = _drivers_comprehension(SIZES, [0, 1])
    assert {d for _c, d in want} == {0, 1} and sorted(c for c, _d in want) == sorted(SIZES)
    assert feed.contig_share(SIZES, [0, 1]) == want
    assert feed.contig_share({}, [0, 1]) == []
    # a rank's share under a process group goes to the rank's own device
    for rank in (0, 1):
        assert feed.contig_share(SIZES, [0], group=(rank, 2, 5)) == [(c, 5) for c in hdist.lpt_assign(SIZES, 2)[rank]]
    # the same through a feed on a BAM with these contigs (no reads: the header is all the assignment looks at)
    bam = str(tmp_path / "empty.bam")
    bamio.write_bam(bam, [batch_from_records(name, length, []) for name, length in SIZES.items()])
    f = feed.ContigFeed(bam, None, None, 1, devices=[0, 1])
    assert f.chrom_lst == ["chr1", "chr2", "chr3", "chr10", "chr11", "chrX"] and f.tname2tsize == SIZES
    assert f.share() == want
    subset = ["chr2", "chr10", "chrX"]
    narrowed = f.share(subset)
    assert narrowed == _drivers_comprehension({c: SIZES[c] for c in subset}, [0, 1])
    assert sorted(c for c, _d in narrowed) == sorted(subset)          # exactly the subset, each contig once
    assert f.share([]) == []
    assert feed.ContigFeed(bam, None, None, 1, devices=()).share() == _drivers_comprehension(SIZES, [0])
    f.close()
