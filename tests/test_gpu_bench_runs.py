"""tools/bench_runs.py's seven runs against the lines the seven scripts it replaces printed on the parent commit
(tests/golden/bench_lines_parent.json: each script once with --contig-len 450000 --depth 30 --steps 2 --warmup 1, three
reference chunks and 900 reads, on which the call run yields 2478 records, so the sites and support runs have sites).

One workload, built here with the reference set, serves all seven runs (the fifteen tests take 0.9 s on an MI355X, the
first 0.4 s of it).  Per run: the new line's keys are a superset of
the recorded ones, recursively; every recorded field that is no time is equal; `reran` is 0; with --wall 3 two
consecutive invocations give the same digest.

A time is a field whose name starts with `ms_` or is a ratio of times (`*_over_*`, `*_GBs`, `*_frac`, `Mbp_per_s`).  The
callable line's `stages` holds four more times under other names (read_pass, map_sweep, compaction, tail): those are not
compared with the recording but must equal the stage means of the same line they are copies of.
"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

RUNS = ("dbs", "indels", "germline", "sites", "support", "bqcal", "callable")
SHAPE = ["--contig-len", "450000", "--depth", "30", "--steps", "2", "--warmup", "1"]

with open(os.path.join(ROOT, "tests", "golden", "bench_lines_parent.json")) as _f:
    GOLDEN = json.load(_f)
_W = []


def workload():
    if not _W:
        import bench_runs
        _W.append(bench_runs.workload(450000, 30.0, True))
    return _W[0]


def line(run, extra=()):
    import bench_runs
    return bench_runs.line(run, workload(), bench_runs.parser().parse_args([run] + SHAPE + list(extra)))


def is_time(name):
    return name.startswith("ms_") or "_over_" in name or name.endswith(("_GBs", "_frac")) or name == "Mbp_per_s"


def compare(new, old, path):
    """Keys of `old` all in `new`, recursively; the fields of `old` that are no times equal."""
    assert set(old) <= set(new), (path, sorted(set(old) - set(new)))
    for k, v in old.items():
        if isinstance(v, dict) and k != "stages":
            compare(new[k], v, path + k + ".")
        elif isinstance(v, dict):
            assert set(v) <= set(new[k]), (path + k, sorted(set(v) - set(new[k])))
        elif not is_time(k):
            assert new[k] == v, (path + k, new[k], v)


def test_recording_is_of_this_shape():
    assert GOLDEN["args"] == " ".join(SHAPE) and sorted(GOLDEN["lines"]) == sorted(RUNS)
    assert GOLDEN["lines"]["sites"]["n_sites"] > 0 and GOLDEN["lines"]["support"]["sites"] > 0


@pytest.mark.parametrize("run", RUNS)
def test_line_is_a_superset_of_the_parent_scripts(run):
    new = json.loads(json.dumps(line(run)))
    compare(new, GOLDEN["lines"][run], run + ":")
    legs = [k for k, v in new.items() if isinstance(v, dict) and "reran" in v]
    assert run in legs and len(legs) == (3 if run == "callable" else 2)
    assert all(new[k]["reran"] == 0 for k in legs)
    assert "digest" not in new and not any(k.startswith("wall") for k in new)
    if run == "callable":
        c = new["callable"]
        assert c["stages"] == {"read_pass": c["ms_index"], "map_sweep": c["ms_eval"], "compaction": c["ms_capture"],
                               "tail": c["ms_finalize"]}


@pytest.mark.parametrize("run", RUNS)
def test_wall_digest_repeats(run):
    first, second = line(run, ["--wall", "3"]), line(run, ["--wall", "3"])
    assert len(first["digest"]) == 40 and first["digest"] == second["digest"]
    assert first["wall_calls"] == 3 and 0 < first["wall_ms_min"] <= first["wall_ms_median"] <= first["wall_ms_max"]
    compare(json.loads(json.dumps(first)), GOLDEN["lines"][run], run + ":")
