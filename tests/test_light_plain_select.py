"""Which light launches run the PLAIN kernels (raingun_amd/csrc/rg_render_launch.h rg_light_plain),
on the CPU: tests/native/light_plain_select_test.cpp, a stand-alone program over hand-built
RgKernelArgs -- every condition flipped once, at 1, 2 and 3 lights.  The header is HIP source,
so hipcc compiles it, host side only (no kernel is instantiated), with AddressSanitizer + UBSan
on that host code (every report fatal); the program runs as a child process.
"""
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "native" / "light_plain_select_test.cpp"
HIPCC = "/opt/rocm/bin/hipcc"
BUILD = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_light_plain_selection(tmp_path):
    exe = tmp_path / "light_plain_select_test"
    subprocess.run([*BUILD, "-o", str(exe), str(SRC)], check=True, timeout=600)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1",
                            "PATH": "/usr/bin:/bin"})
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"
