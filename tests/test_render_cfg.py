"""The render kernel's configuration, grid arithmetic and light-batch ladder on the CPU
(raingun_amd/csrc/rg_render_cfg.h, rg_render_grid.h, rg_render_launch.h):
tests/native/render_cfg_test.cpp, a stand-alone program of static_asserts on RenderCfg for one kernel
of each kind and of hand-worked grid cases.  Compiled as tests/test_light_plain_select.py compiles
its program -- hipcc, host side only (no kernel is instantiated), AddressSanitizer + UBSan on that
host code (every report fatal) -- and run as a child process.  Also: scripts/render_kernel_name.py,
the mangled-name helper of the profiling scripts, round trip.
"""
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "native" / "render_cfg_test.cpp"
HIPCC = "/opt/rocm/bin/hipcc"
BUILD = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_render_cfg_and_grid(tmp_path):
    exe = tmp_path / "render_cfg_test"
    subprocess.run([*BUILD, "-o", str(exe), str(SRC)], check=True, timeout=600)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1",
                            "PATH": "/usr/bin:/bin"})
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"


def test_render_kernel_name_round_trip():
    sys.path.insert(0, str(REPO / "scripts"))
    try:
        import render_kernel_name as rkn
    finally:
        sys.path.pop(0)
    headline = "_Z16rg_render_kernelILi8ELb1ELb1ELi4ELi3ELb0ELb0ELb0ELi0ELb0ELb0ELb1EEv12RgKernelArgs"
    assert rkn.HEADLINE == headline
    p = rkn.parse(headline)
    assert p == dict(MAXD=8, LSPH=True, LCOLD=True, WPS=4, LBT=3, F32F=False, BVH=False, TASKS=False, TPW=0,
                     HF=False, SPARSE=False, PLAIN=True)
    assert rkn.describe(p) == "light plain"
    # negative values (the one-light batch, persistent waves) are mangled with an 'n'
    one = "_Z16rg_render_kernelILi8ELb1ELb1ELi4ELin1ELb0ELb0ELb0ELin1ELb0ELb0ELb0EEv12RgKernelArgs"
    assert rkn.parse(one)["LBT"] == -1 and rkn.parse(one)["TPW"] == -1
    assert rkn.describe(rkn.parse(one)) == "light tpw=-1"
    heavy = rkn.mangle(MAXD=8, LSPH=True, LCOLD=False, WPS=3, LBT=1, F32F=True, BVH=True, TASKS=True, TPW=0, HF=True,
                       SPARSE=False, PLAIN=False)
    assert heavy == "_Z16rg_render_kernelILi8ELb1ELb0ELi3ELi1ELb1ELb1ELb1ELi0ELb1ELb0ELb0EEv12RgKernelArgs"
    assert rkn.describe(rkn.parse(heavy)) == "heavy host"
    for name in (headline, one, heavy):
        assert rkn.mangle(**rkn.parse(name)) == name
    assert rkn.parse("_Z15rg_trace_kernelv") is None
