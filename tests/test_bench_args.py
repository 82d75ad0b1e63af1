"""bench.py's command line, checked before any GPU call: --steps sets the timed steps (at least one), and the per-GEMM
table belongs to the --full run that measures the roofline."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("argv,msg", [(["--steps", "0"], "--steps must be >= 1"),
                                      (["--gemm-shapes", "x.jsonl"], "--gemm-shapes needs the roofline step"),
                                      (["--full", "--no-roofline", "--gemm-shapes", "x.jsonl"], "--gemm-shapes needs")])
def test_bench_rejects_inconsistent_flags(argv, msg):
    r = subprocess.run([sys.executable, "bench.py"] + argv, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and msg in r.stderr, r.stderr[-2000:]


def test_bench_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, "bench.py", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs DIR" in r.stdout
