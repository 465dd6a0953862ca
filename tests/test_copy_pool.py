"""The pageable-frame copy pool (raingun_amd/csrc/rg_copy_pool.cpp) on the CPU:
tests/native/copy_pool_test.cpp, a stand-alone program, built once with
ThreadSanitizer and once with AddressSanitizer + UBSan (every report fatal)
and run as a child process.  The pool is the library's only lock-free threaded
host code; on the GPU it runs only under pageable-destination renders.
"""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
SRC = [REPO / "tests" / "native" / "copy_pool_test.cpp", REPO / "raingun_amd" / "csrc" / "rg_copy_pool.cpp"]
BASE = ["g++", "-std=c++17", "-O1", "-g", "-pthread"]
BUILDS = {"tsan": ["-fsanitize=thread"],
          "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("name", sorted(BUILDS))
def test_copy_pool_under_sanitizer(name, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = tmp_path / f"copy_pool_{name}"
    subprocess.run([*BASE, *BUILDS[name], "-o", str(exe), *map(str, SRC)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={"TSAN_OPTIONS": "halt_on_error=1", "ASAN_OPTIONS": "detect_leaks=1",
                            "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"})
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"
