"""Randomised parity of the germline run with the model of its contract through ONE context (tools/fuzz_parity.py
--germline): contigs of changing length, depth, error rates and read lengths, regions in any order, thresholds, zero
qualities and bases outside ATGC in some, a call run against the oracle between some of the rounds."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_germline_fuzz_through_one_context():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_parity.py"), "--germline", "--seed", "3", "--rounds", "36",
                        "--minutes", "3"], capture_output=True, text=True, timeout=400)
    tail = "\n".join(r.stdout.splitlines()[-6:])
    assert r.returncode == 0 and "fuzz ok" in r.stdout, tail + r.stderr[-2000:]
    assert sum(l.startswith("ok") for l in r.stdout.splitlines()) >= 12, tail
