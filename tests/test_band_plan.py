"""The band arithmetic of the host-visible and the supersampled frames
(raingun_amd/csrc/rg_band_plan.h, no HIP in it) on the CPU:
tests/native/band_plan_test.cpp, a stand-alone program, built with
AddressSanitizer + UBSan (every report fatal) and run as a child process.
"""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "native" / "band_plan_test.cpp"
BUILD = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_band_plan_under_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = tmp_path / "band_plan_test"
    subprocess.run([*BUILD, "-o", str(exe), str(SRC)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1",
                            "PATH": "/usr/bin:/bin"})
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"
