"""The exact replacements the PLAIN light kernels use for divisions by launch constants
(raingun_amd/csrc/rg_exact.h), on the CPU: tests/native/exact_div_test.cpp, a stand-alone program
over the header alone, compiled with g++ -O2 -ffp-contract=off (C fma, no contraction) --

  * the camera quotient (i + 0.5) / n from 1.0 / n, for every n <= 20000 and every i < n, bit for bit;
    rg_recip_div_ok true for each of those n, false with a reciprocal an ulp off;
  * the texture wrap (i32 % dimension, then + dimension below zero) and the unsigned quotient under
    it from the divisor's magic: divisors 1..4096, 2^k and 2^k +- 1 up to 2^30, 2^31 - 1, the golden
    textures' sides; dividends i32::MIN, MIN + 1, MAX, every value within 1 of a multiple of the
    divisor near 0 and near +-2^31, 100,000 seeded random ones;
  * the host's plane texture axes against texture_coords' expressions, bit for bit;
  * the camera ray's range predicate --

and tests/native/light_plain_exact_select_test.cpp: the conditions the launcher's PLAIN predicate
gained (hipcc, host side only, as tests/test_light_plain_select.py builds its program).
"""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
NATIVE = REPO / "tests" / "native"
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def exact_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("exact_div") / "exact_div_test"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                    str(NATIVE / "exact_div_test.cpp"), "-lm"], check=True, timeout=300)
    return exe


@pytest.mark.parametrize("part", ["quotients", "modulo", "axes", "camera"])
def test_exact_replacements(exact_exe, part):
    p = subprocess.run([str(exact_exe), part], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_light_plain_exact_conditions(tmp_path):
    exe = tmp_path / "light_plain_exact_select_test"
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                    "-o", str(exe), str(NATIVE / "light_plain_exact_select_test.cpp")], check=True, timeout=600)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"
