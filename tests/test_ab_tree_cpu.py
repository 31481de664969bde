"""tools/ab.py --tree: builds that are checkouts of their own -- each child runs from its build's directory with its own
Python and library, nothing of the environment changed -- alternated and reported like --lib builds."""
import io
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import ab  # noqa: E402

CHILD = """
import json, os, sys
with open(sys.argv[1], "a") as f:
    f.write(json.dumps({"cwd": os.getcwd(), "lib": os.environ.get("HIMUT_HIP_LIB_OVERRIDE")}) + chr(10))
print(json.dumps({"ms_per_step": 1.0 if os.path.basename(os.getcwd()) == "parent" else 1.5}))
"""


def test_tree_builds_run_from_their_own_directory(tmp_path, monkeypatch):
    monkeypatch.delenv("HIMUT_HIP_LIB_OVERRIDE", raising=False)
    monkeypatch.chdir(tmp_path)
    (tmp_path / "parent").mkdir()
    (tmp_path / "this").mkdir()
    log = str(tmp_path / "children.log")
    a = ab.parser().parse_args(["--tree", "parent=parent", "--tree", "this=" + str(tmp_path / "this"), "--bench", "x", "--rounds", "2"])
    assert ab.builds_of(a) == [("parent", {ab.CWD: str(tmp_path / "parent")}), ("this", {ab.CWD: str(tmp_path / "this")})]
    printed = io.StringIO()
    status = ab.drive(a, command=lambda bench, a: ([sys.executable, "-c", CHILD, log], 7), out=printed)
    assert status == 0
    seen = [json.loads(s) for s in open(log).read().splitlines()]
    assert [os.path.basename(s["cwd"]) for s in seen] == ["parent", "this", "parent", "this"]
    assert all(s["lib"] is None for s in seen)
    assert "| x `ms_per_step` | 1.0000 (1.0000–1.0000) | 1.5000 (1.5000–1.5000) | NO |" in printed.getvalue()


def test_without_a_tree_the_children_run_from_the_repository(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    log = str(tmp_path / "children.log")
    a = ab.parser().parse_args(["--bench", "x", "--rounds", "1"])
    assert ab.builds_of(a) == [("default", {})]
    assert ab.drive(a, command=lambda bench, a: ([sys.executable, "-c", CHILD, log], 7), out=io.StringIO()) == 0
    assert json.loads(open(log).read())["cwd"] == ab.ROOT
