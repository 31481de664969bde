#!/usr/bin/env python3
"""Regenerates tests/golden/bqcal_*.json: the per-quality match and mismatch counts of the REFERENCE's own worker,
get_bq2match_mismatch_count of its scripts/ccs2bq_calculation.py, run through tests/golden/ref_harness.py on the reads
and the contig strings the norm_*.npz fixtures already hold.

Run in the build container only:  python tests/golden/make_golden_bqcal.py
The script is loaded from the reference checkout by path; none of its text is here.  The outputs hold the parameters
and the 93 + 93 counts, nothing else; the tests never need the reference."""
import json
import os
import sys

_FEATS = "AVX512F AVX512CD AVX512VL AVX512BW AVX512DQ AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR AVX2 FMA3"
if os.environ.get("NPY_DISABLE_CPU_FEATURES") != _FEATS:
    # numpy must come up with its SIMD sorts off so np.argsort breaks ties the way the numpy pinned by the reference
    # does: as make_golden.py
    env = dict(os.environ, NPY_DISABLE_CPU_FEATURES=_FEATS)
    import subprocess
    sys.exit(subprocess.call([sys.executable] + sys.argv, env=env))

import importlib.util  # noqa: E402

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_harness as H  # noqa: E402
from himut_amd.readbatch import ReadBatch  # noqa: E402

SCRIPT = os.path.join(os.path.dirname(H.REFERENCE_SRC), "scripts", "ccs2bq_calculation.py")

# case -> (fixture with the reads and refseq, regions or None for the fixture's chunks, md_threshold or None for the
# fixture's, min_gq, germline_snv_prior)
CASES = {
    "bqcal_basic": ("norm_basic", None, None, 20, 1 / (10 ** 3)),
    "bqcal_dense": ("norm_dense", None, None, 20, 1 / (10 ** 3)),
    "bqcal_softmask": ("norm_softmask", None, None, 20, 1 / (10 ** 3)),
    "bqcal_insins": ("norm_insins", None, None, 20, 1 / (10 ** 3)),
    # a lower depth bar than the fixture's 60 (its piles are about 70 deep), a higher GQ bar, another prior
    "bqcal_dense_md": ("norm_dense", None, 55, 40, 1 / (10 ** 2)),
    # three regions whose borders fall inside reads, off every tile grid; a gap between the last two
    "bqcal_basic_regions": ("norm_basic", [(137, 9411), (9411, 20003), (26500, 39871)], None, 20, 1 / (10 ** 3)),
}


def load_script():
    H.load_reference()
    spec = importlib.util.spec_from_file_location("ccs2bq_calculation", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    script = load_script()
    for case, (fixture, regions, md, min_gq, prior) in CASES.items():
        with open(os.path.join(HERE, fixture + ".json")) as f:
            fx = json.load(f)
        with np.load(os.path.join(HERE, fixture + ".npz")) as z:
            batch = ReadBatch.from_npz_dict(z)
            seq = bytes(z["refseq"]).decode("ascii")
        regions = [tuple(c) for c in (fx["chunks"] if regions is None else regions)]
        md = fx["md_threshold"] if md is None else md
        bam = "/fake/{}.bam".format(case)
        H.register_bam(bam, {batch.name: batch})
        match, mismatch = {}, {}
        script.get_bq2match_mismatch_count(batch.name, [(batch.name, s, e) for s, e in regions], bam, seq, min_gq, md, prior,
                                           match, mismatch)
        exp = {"fixture": fixture, "regions": [list(r) for r in regions], "md_threshold": int(md), "min_gq": int(min_gq),
               "germline_snv_prior": prior,
               "match": [int(match[batch.name][bq]) for bq in range(1, 94)],
               "mismatch": [int(mismatch[batch.name][bq]) for bq in range(1, 94)]}
        with open(os.path.join(HERE, case + ".json"), "w") as o:
            json.dump(exp, o, sort_keys=True)
            o.write("\n")
        print("wrote", case, "match", sum(exp["match"]), "mismatch", sum(exp["mismatch"]),
              "bins", sum(1 for v in exp["mismatch"] if v))


if __name__ == "__main__":
    main()
