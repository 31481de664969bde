"""tools/bench_runs.py's skeleton (alternate, summarise) and tools/ab.py's driver on stand-in children that open no GPU."""
import io
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ab  # noqa: E402
import bench_runs  # noqa: E402


def numbered(name, seen):
    """A stand-in step: returns {"leg", "n"} with n counting this leg's calls, and notes the call in `seen`."""
    count = [0]

    def step():
        seen.append(name)
        count[0] += 1
        return {"leg": name, "n": count[0]}
    return step


@pytest.mark.parametrize("steps,warmup", [(3, 2), (1, 0), (4, 1)])
def test_alternate_two_legs(steps, warmup):
    seen = []
    acc = bench_runs.alternate([("call", numbered("call", seen)), ("dbs", numbered("dbs", seen))], steps, warmup)
    assert seen == ["call", "dbs"] * (steps + warmup)
    assert list(acc) == ["call", "dbs"]
    for name in ("call", "dbs"):
        assert acc[name] == [{"leg": name, "n": k} for k in range(warmup + 1, warmup + steps + 1)]


def test_alternate_three_legs_in_the_callable_order():
    seen = []
    order = ["normcounts", "normcounts_tile", "callable"]
    acc = bench_runs.alternate([(n, numbered(n, seen)) for n in order], 2, 1)
    assert seen == order * 3
    assert list(acc) == order
    assert all(acc[n] == [{"leg": n, "n": 2}, {"leg": n, "n": 3}] for n in order)


def test_summarise_by_hand():
    def row(total, parse, reran, records, cand, slots):
        return {"ms_total": total, "ms_parse": parse, "ms_index": 0.5, "ms_capture": 2.0 * total, "ms_emit": 0.0, "ms_eval": 1.0,
                "ms_finalize": 0.25, "reran": reran, "n_records": records, "n_candidates": cand, "column_slots": slots}
    rows = [row(4.0, 1.0, 0, 7, 70, 700), row(1.0, 2.0, 1, 8, 80, 800), row(2.0, 6.0, 0, 9, 90, 900), row(9.0, 3.0, 2, 10, 100, 1000)]
    d = bench_runs.summarise(rows)
    assert d == {"ms_total": 4.0, "ms_parse": 3.0, "ms_index": 0.5, "ms_capture": 8.0, "ms_emit": 0.0, "ms_eval": 1.0, "ms_finalize": 0.25,
                 "ms_total_min": 1.0, "ms_total_max": 9.0, "ms_total_median": 3.0, "reran": 3,
                 "records": 10, "candidates": 100, "column_slots": 1000}
    assert bench_runs.summarise(rows[:3])["ms_total_median"] == 2.0


def test_commands_and_time_limits():
    a = ab.parser().parse_args(["--legs=", "--wall", "30"])
    assert ab.command("call", a) == (["python3", "bench.py", "--full", "--no-cpu-baseline", "--steps", "40", "--warmup", "10", "--legs="], 200)
    assert ab.command("dbs", a) == (["python3", "tools/bench_runs.py", "dbs", "--wall", "30"], 200)
    k = ab.parser().parse_args(["--kstats", "k_norm_", "--bench-args=--error-rate 5e-4"])
    assert ab.command("call", k) == (["python3", "bench.py", "--steps", "10", "--warmup", "3", "--no-cpu-baseline"], 300)
    assert ab.command("normcounts", k) == (["python3", "tools/bench_normcounts.py", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
                                            "--error-rate", "5e-4"], 100)
    assert ab.command("callable", ab.parser().parse_args(["--kstats", "k_call"])) == (["python3", "tools/bench_runs.py", "callable"], 300)


# a child of the driver: notes its environment in the log, prints a line of noise and its JSON line, ends with the status
# of its turn (the number of children before it is the log's length)
CHILD = """
import json, os, sys
log, statuses, total, evals = sys.argv[1], json.loads(sys.argv[2]), json.loads(sys.argv[3]), json.loads(sys.argv[4])
n = len(open(log).read().splitlines()) if os.path.exists(log) else 0
with open(log, "a") as f:
    f.write(json.dumps({"lib": os.environ.get("HIMUT_HIP_LIB_OVERRIDE"), "var": os.environ.get("AB_TEST_VAR")}) + chr(10))
print("not the line")
print(json.dumps({"run": {"ms_total": total[n], "ms_eval": evals[n], "ms_total_max": 99.0, "reran": 0, "records": 5}, "digest": "d0"}))
sys.exit(statuses[n])
"""
TOTAL = [1.0, 2.0, 3.0, 5.0]           # build a: 1, 3 -> median 2 (1-3); build b: 2, 5 -> median 3.5 (2-5), outside a's range
EVALS = [4.0, 4.5, 6.0, 5.5]           # build a: 4, 6 -> median 5 (4-6); build b: 4.5, 5.5 -> median 5, inside


def run_driver(tmp_path, monkeypatch, argv, statuses):
    """The driver on stand-in children; (status, printed text, the children's log, the JSONL objects, the calls made)."""
    log, out = str(tmp_path / "children.log"), str(tmp_path / "out.jsonl")
    calls = []
    real = subprocess.run

    def recording(cmd, **kw):
        calls.append((cmd, kw["env"]))
        return real(cmd, **kw)
    monkeypatch.setattr(ab.subprocess, "run", recording)

    def command(bench, a):
        return [sys.executable, "-c", CHILD, log, json.dumps(statuses), json.dumps(TOTAL), json.dumps(EVALS)], 7
    a = ab.parser().parse_args(argv + ["--bench", "x", "--rounds", "2", "--out", out])
    printed = io.StringIO()
    status = ab.drive(a, command=command, out=printed)
    seen = [json.loads(s) for s in open(log).read().splitlines()]
    lines = [json.loads(s) for s in open(out).read().splitlines()] if os.path.exists(out) else []
    return SimpleNamespace(status=status, text=printed.getvalue(), seen=seen, lines=lines, calls=calls)


def test_ab_alternates_builds_and_reports_medians(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    r = run_driver(tmp_path, monkeypatch, ["--lib", "a=some/dir/a.so", "--lib", "b=" + str(tmp_path / "b.so")], [0, 0, 0, 0])
    assert r.status == 0
    lib_a, lib_b = str(tmp_path / "some" / "dir" / "a.so"), str(tmp_path / "b.so")
    assert [s["lib"] for s in r.seen] == [lib_a, lib_b, lib_a, lib_b]
    assert all(os.path.isabs(env["HIMUT_HIP_LIB_OVERRIDE"]) for _, env in r.calls)
    assert all(cmd[:4] == ["timeout", "-k", "10", "7"] for cmd, _ in r.calls) and len(r.calls) == 4
    assert [(o["bench"], o["build"], o["round"]) for o in r.lines] == [("x", "a", 1), ("x", "b", 1), ("x", "a", 2), ("x", "b", 2)]
    assert [o["line"]["run"]["ms_total"] for o in r.lines] == TOTAL
    assert [o["line"]["run"]["ms_eval"] for o in r.lines] == EVALS
    assert all(sorted(o) == ["bench", "build", "line", "round"] and o["line"]["digest"] == "d0" for o in r.lines)
    assert "| x `run.ms_total` | 2.0000 (1.0000–3.0000) | 3.5000 (2.0000–5.0000) | NO |" in r.text
    assert "| x `run.ms_eval` | 5.0000 (4.0000–6.0000) | 5.0000 (4.5000–5.5000) | yes |" in r.text
    assert "ms_total_max" not in r.text
    assert "digest of x: equal in all 4 lines (d0)" in r.text
    assert "reran: 0 over 4 lines" in r.text


def test_ab_env_sets_and_unsets(tmp_path, monkeypatch):
    monkeypatch.setenv("AB_TEST_VAR", "outer")
    monkeypatch.delenv("HIMUT_HIP_LIB_OVERRIDE", raising=False)
    r = run_driver(tmp_path, monkeypatch, ["--env", "AB_TEST_VAR=-,v"], [0, 0, 0, 0])
    assert r.status == 0
    assert [s["var"] for s in r.seen] == [None, "v", None, "v"]
    assert ["AB_TEST_VAR" in env for _, env in r.calls] == [False, True, False, True]
    assert all(s["lib"] is None for s in r.seen)
    assert [o["build"] for o in r.lines] == ["AB_TEST_VAR=-", "AB_TEST_VAR=v"] * 2


@pytest.mark.parametrize("statuses,ran", [([0, 0, 3, 0], 3), ([0, 124, 0, 0], 2), ([137, 0, 0, 0], 1)])
def test_ab_stops_at_the_first_failed_child(tmp_path, monkeypatch, statuses, ran):
    r = run_driver(tmp_path, monkeypatch, ["--lib", "a=a.so", "--lib", "b=b.so"], statuses)
    assert r.status != 0
    assert len(r.seen) == ran and len(r.calls) == ran
    assert [o["line"]["run"]["ms_total"] for o in r.lines] == TOTAL[:ran - 1]
    assert "status {}".format(statuses[ran - 1]) in r.text and "nothing more is started" in r.text
    assert "|" not in r.text
