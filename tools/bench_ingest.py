#!/usr/bin/env python3
"""Host ingest rate: writes a synthetic 30x BAM for a contig of --contig-len, then times bamio.BamFile() with 1, 4, 8,
16 inflate threads.  CPU only.

--derive_cs (needs the GPU): the device-side ingest of the bench BAM (tools/bench_e2e.py's: seed 3, 30x, 64.4 Mb unless
--contig-len says otherwise) with its cs tags, and again deriving the cs text from CIGAR, SEQ and the reference
(himut_ingest_derive_cs): wall seconds of both, the device milliseconds of the post-pass (himut_ingest_derive_result,
out[3]; its exact figure with HIMUT_INGEST_PROFILE=1 on stderr), the post-pass's algorithmic bytes -- both walks read
half a byte of SEQ and a byte of reference per aligned column, the second writes the text -- and their share of the HBM
peak."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contig-len", type=int, default=None)
    ap.add_argument("--derive_cs", action="store_true")
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    if a.derive_cs:
        return derive_cs(a.contig_len or 64_444_167, a.repeat)
    a.contig_len = a.contig_len or 16_000_000
    from himut_amd import bamio, synth
    s = synth.generate(synth.SynthConfig(seed=3, contig_len=a.contig_len, name="chr1"))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "x.bam")
        bamio.write_bam(path, [s.batch])
        size = os.path.getsize(path)
        payload = s.batch.seq.nbytes + s.batch.bq.nbytes + s.batch.cs.nbytes
        out = {"bam_MB": size / 1e6, "payload_MB": payload / 1e6, "reads": int(s.batch.n), "runs": []}
        for th in (1, 4, 8, 16):
            best = 1e9
            for _ in range(2):
                t = time.perf_counter()
                bamio.BamFile(path, th)
                best = min(best, time.perf_counter() - t)
            out["runs"].append({"threads": th, "seconds": best, "bam_MB_per_s": size / 1e6 / best,
                                "read_Mbases_per_s": s.batch.total_read_bases() / 1e6 / best})
    print(json.dumps(out))


HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak, as bench.py has it


def derive_cs(contig_len, repeat):
    import numpy as np
    from himut_amd import bamio, caller, synth
    s = synth.generate(synth.SynthConfig(seed=3, contig_len=contig_len, name="chr20"), want_ref=True)
    ref = bytes(s.ref)
    want_cs = s.batch.cs.copy()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "x.bam")
        bamio.write_bam(path, [s.batch], sample="SMP")
        del s
        for rep in range(repeat):
            w = caller.Worker(0)
            t = {"repeat": rep, "contig_Mb": contig_len / 1e6, "bam_MB": os.path.getsize(path) / 1e6}
            for mode in (0, 1):
                st = bamio.BamStream(path, 0)
                if mode:
                    t0 = time.perf_counter()
                    bamio.set_contig_reference(w.ctx, ref)
                    t["set_reference_s"] = time.perf_counter() - t0
                t0 = time.perf_counter()
                res = st.ingest_contig(w.ctx, "chr20", derive_cs=bool(mode))
                t["ingest_derive_s" if mode else "ingest_tags_s"] = time.perf_counter() - t0
                st.close()
            r = w.ctx.ingest_derive_result()
            ts, te = w.ctx.ingest_read_meta(res["n_reads"])[:2]
            span = int((te.astype(np.int64) - ts).sum())
            alg = 2 * (res["read_bases"] // 2 + span) + r["cs_bytes"]
            t.update(post_pass_device_ms=r["ms"], derived=r["n_derived"], underivable=r["n_underivable"],
                     cs_bytes=r["cs_bytes"], algorithmic_bytes=alg, reads=res["n_reads"], read_bases=res["read_bases"])
            if r["ms"]:
                t["achieved_GB_per_s"] = alg / (r["ms"] / 1e3) / 1e9
                t["frac_of_hbm_peak"] = t["achieved_GB_per_s"] / HBM_PEAK_GBS
            if rep == 0:
                got = w.ctx.download_reads(res, "chr20", contig_len)
                t["text_equals_the_tags"] = bool(np.array_equal(got.cs, want_cs))
            w.close()
            print(json.dumps(t), flush=True)


if __name__ == "__main__":
    main()
