#!/usr/bin/env python3
"""Builds of the library, or settings of an environment variable, alternated on one box: every measurement is a fresh
child process under a time limit of its own, one at a time, first build first within a round.  The first child that does
not end with status 0 ends the whole call: nothing more is started on the GPU, the lines gathered so far stay in --out.

    python tools/ab.py --rounds 5 --lib parent=<a.so> --lib this=<b.so> --bench call --bench dbs --bench indels \\
        [--wall 30] --out profiles/<name>.jsonl
    python tools/ab.py --rounds 3 --env VAR=-,value --bench call                   # "-" = the variable unset
    python tools/ab.py --rounds 3 --tree parent=<checkout> --tree this=. --bench call   # each with its own Python and library:
                                                                                   # for a change that adds entry points
    python tools/ab.py --kstats 'k_norm_|k_callable' --bench normcounts --lib ...  # rocprofv3 kernel averages

Bench `call` is bench.py's call step, `normcounts` tools/bench_normcounts.py, `spectra` tools/bench_spectra.py, `fit` tools/bench_fit.py, every other
name a run of tools/bench_runs.py.  One JSON object per child goes to --out ({"bench", "build", "round", "line"}); at the end a table:
per bench and time field the median with (min-max) over the rounds for each build, whether the last build's median lies
inside the first build's range, and whether the digests of --wall are equal across the builds.
"""
import argparse
import csv
import glob
import json
import os
import re
import shlex
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = {"call": (200, 300), "normcounts": (100, 100)}     # seconds: the bench alone, under rocprofv3
LIMIT_S_OTHER = (200, 300)
CWD = "(cwd)"                          # a build's setting that is the child's directory, not a variable (--tree)
TIME_FIELD = re.compile(r"(^|_)(ms|us)(_|$)")


def kstats(directory):
    """The per-kernel rows of a rocprofv3 --kernel-trace --stats run: [(name, calls, average us)]."""
    hits = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    with open(hits[0]) as f:
        return [(r["Name"], int(r["Calls"]), float(r["AverageNs"]) / 1e3) for r in csv.DictReader(f)]


def command(bench, a):
    """(argv of the child, its time limit in seconds) for one bench; under --kstats the short runs the traces use."""
    extra = shlex.split(a.bench_args)
    if bench == "call":
        argv = ["bench.py", "--steps", "10", "--warmup", "3", "--no-cpu-baseline"] if a.kstats else \
               ["bench.py", "--full", "--no-cpu-baseline", "--steps", "40", "--warmup", "10"]
        argv += [] if a.legs is None else ["--legs=" + a.legs]
    elif bench == "normcounts":
        argv = ["tools/bench_normcounts.py", "--steps", "3", "--warmup", "1", "--no-cpu-baseline"] + extra
    elif bench == "spectra":
        argv = ["tools/bench_spectra.py"] + extra
    elif bench == "fit":
        argv = ["tools/bench_fit.py"] + extra
    else:
        argv = ["tools/bench_runs.py", bench] + (["--wall", str(a.wall)] if a.wall else []) + extra
    return ["python3"] + argv, LIMIT_S.get(bench, LIMIT_S_OTHER)[1 if a.kstats else 0]


def builds_of(a):
    """[(name, {variable: value, or None for unset})]: the libraries and the trees (CWD: the directory), the settings of
    --env, or their product."""
    libs = [(n, {"HIMUT_HIP_LIB_OVERRIDE": os.path.abspath(p)}) for n, p in (s.split("=", 1) for s in a.lib)] + \
           [(n, {CWD: os.path.abspath(p)}) for n, p in (s.split("=", 1) for s in a.tree)] or [("", {})]
    envs = [("", {})]
    if a.env:
        var, values = a.env.split("=", 1)
        envs = [("{}={}".format(var, v), {var: None if v == "-" else v}) for v in values.split(",")]
    return [(",".join(x for x in (ln, en) if x) or "default", dict(le, **ee)) for ln, le in libs for en, ee in envs]


def time_fields(line, prefix=""):
    """dotted path -> value of the numeric leaves that are times (a component of the path has the word ms or us)."""
    out = {}
    for k, v in line.items():
        path = prefix + k
        if isinstance(v, dict):
            out.update(time_fields(v, path + "."))
        elif isinstance(v, (int, float)) and not isinstance(v, bool) and any(TIME_FIELD.search(p) for p in path.split(".")) \
                and not path.endswith(("_min", "_max")):
            out[path] = float(v)
    return out


def table(results, builds, field=None):
    """The lines of the closing table; results: [{"bench", "build", "round", "line"}]."""
    names = [n for n, _ in builds]
    lines = ["| | " + " | ".join(names) + " | last median inside the first's range |", "|---|" + "---|" * (len(names) + 1)]
    for bench in dict.fromkeys(r["bench"] for r in results):
        per = {n: [time_fields(r["line"]) for r in results if r["bench"] == bench and r["build"] == n] for n in names}
        for f in (f for f in per[names[0]][0] if not field or re.search(field, f)):
            vals = {n: [row[f] for row in per[n] if f in row] for n in names}
            if not all(vals.values()):
                continue
            cells = ["{:.4f} ({:.4f}–{:.4f})".format(statistics.median(v), min(v), max(v)) for v in vals.values()]
            first, last = vals[names[0]], vals[names[-1]]
            lines.append("| {} `{}` | {} | {} |".format(bench, re.sub(r"\(.*\)", "", f), " | ".join(cells),   # a kernel without its arguments
                                                        "yes" if min(first) <= statistics.median(last) <= max(first) else "NO"))
        digests = {r["line"]["digest"] for r in results if r["bench"] == bench and "digest" in r["line"]}
        if digests:
            lines.append("digest of {}: {}".format(bench, "equal in all {} lines ({})".format(
                sum(r["bench"] == bench for r in results), min(digests)) if len(digests) == 1 else "DIFFERENT: " + " ".join(sorted(digests))))
    reran = sum(int(v.get("reran", 0)) for r in results for v in r["line"].values() if isinstance(v, dict))
    lines.append("reran: {} over {} lines".format(reran, len(results)))
    return lines


def drive(a, command=command, out=sys.stdout):
    """Runs the children; returns the exit status of the call."""
    builds, results = builds_of(a), []
    for rnd in range(1, a.rounds + 1):
        for bench in a.bench:
            for name, setting in builds:
                argv, limit = command(bench, a)
                env = dict(os.environ)
                for var, value in setting.items():
                    if var == CWD:
                        continue
                    env.pop(var, None)
                    if value is not None:
                        env[var] = value
                trace = None
                if a.kstats:                   # kernel tracing alone: counters are collected in runs of their own
                    trace = tempfile.mkdtemp(prefix="ab_kstats_")
                    env["TMPDIR"] = "/tmp"
                    argv = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "--"] + argv
                p = subprocess.run(["timeout", "-k", "10", str(limit)] + argv, cwd=setting.get(CWD, ROOT), env=env, stdout=subprocess.PIPE,
                                   stderr=subprocess.PIPE, universal_newlines=True)
                line = None
                if p.returncode == 0:
                    try:
                        if trace:
                            line = {"kernels": {k: {"calls": c, "avg_us": us} for k, c, us in kstats(trace) if re.search(a.kstats, k)}}
                        else:
                            line = json.loads(p.stdout.strip().splitlines()[-1])
                    except (IndexError, ValueError) as e:
                        print("{} {} round {}: no result to read ({})".format(bench, name, rnd, e), file=out)
                if trace:
                    shutil.rmtree(trace, ignore_errors=True)
                if line is None:               # fail-stop: no retry, no next build
                    print("{} {} round {}: child ended with status {}; nothing more is started".format(bench, name, rnd, p.returncode),
                          file=out)
                    print("\n".join(p.stderr.splitlines()[-20:]), file=out)
                    return p.returncode if 0 < p.returncode < 256 else 1
                results.append({"bench": bench, "build": name, "round": rnd, "line": line})
                print("{} {} round {}: ok".format(bench, name, rnd), file=out, flush=True)
                if a.out:
                    with open(a.out, "a") as o:
                        o.write(json.dumps(results[-1]) + "\n")
    print("\n".join(table(results, builds, a.field)), file=out)
    return 0


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lib", action="append", default=[], metavar="NAME=PATH", help="a build of the library (HIMUT_HIP_LIB_OVERRIDE)")
    ap.add_argument("--tree", action="append", default=[], metavar="NAME=DIR",
                    help="a checkout with its own build: the bench runs from there, with that tree's Python and library")
    ap.add_argument("--env", default=None, metavar="VAR=A,B", help="settings of one environment variable, - = unset")
    ap.add_argument("--bench", action="append", default=[], help="call, normcounts, or a run of tools/bench_runs.py")
    ap.add_argument("--legs", default=None, help="bench.py's --legs for bench call (empty: the call step alone)")
    ap.add_argument("--wall", type=int, default=0, help="--wall of tools/bench_runs.py")
    ap.add_argument("--bench-args", default="", help="further arguments of the tools' command lines, as one string")
    ap.add_argument("--kstats", default=None, metavar="REGEX", help="run under rocprofv3 --kernel-trace --stats; the kernels that match")
    ap.add_argument("--field", default=None, metavar="REGEX", help="the table's fields (default: every time field)")
    ap.add_argument("--out", default=None, help="append one JSON object per child to this file")
    return ap


if __name__ == "__main__":
    args = parser().parse_args()
    args.bench = args.bench or ["call"]
    sys.exit(drive(args))
