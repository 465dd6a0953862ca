"""The merge of per-pass statistics and the statuses that still deliver a frame
(raingun_amd/csrc/rg_stats_merge.h, no HIP in it) on the CPU: tests/native/stats_merge_test.cpp,
a stand-alone program, built with AddressSanitizer + UBSan (every report fatal) and run as a
child process.
"""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "native" / "stats_merge_test.cpp"
BUILD = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
ENV = {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    out = tmp_path_factory.mktemp("stats_merge") / "stats_merge_test"
    subprocess.run([*BUILD, "-o", str(out), str(SRC)], check=True)
    return out


def test_stats_merge_under_sanitizer(exe):
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=ENV)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"
