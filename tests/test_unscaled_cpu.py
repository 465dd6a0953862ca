"""The per-lane admission of the PLAIN light kernels' unscaled f64 sqrt / division
(raingun_amd/csrc/rg_exact.h), on the CPU: tests/native/unscaled_test.cpp, a stand-alone
program over the header alone, compiled with g++ -O2 -ffp-contract=off like tests/test_exact_div.py's --
the window predicate on every biased exponent with zero, all-ones and random mantissas, both signs,
the edge values 2^-256 and 2^257 and their neighbours, and the excluded classes (zeros, denormals,
infinities, NaNs, negatives for sqrt).
"""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
NATIVE = REPO / "tests" / "native"


@pytest.fixture(scope="module")
def unscaled_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("unscaled") / "unscaled_test"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                    str(NATIVE / "unscaled_test.cpp"), "-lm"], check=True, timeout=300)
    return exe


def test_unscaled_window(unscaled_exe):
    p = subprocess.run([str(unscaled_exe), "window"], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"
