"""The dealing of tiles to ranks and devices (raingun_amd/csrc/rg_tile_deal.h, no HIP
in it) on the CPU: tests/native/tile_deal_test.cpp, a stand-alone program, built with
AddressSanitizer + UBSan (every report fatal) and run as a child process; and its deal
of a list of cases against the Python statement of it (raingun_amd/distributed.py).
"""
import shutil
import subprocess
from pathlib import Path

import pytest

from raingun_amd import distributed as rd

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "native" / "tile_deal_test.cpp"
BUILD = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
ENV = {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    out = tmp_path_factory.mktemp("tile_deal") / "tile_deal_test"
    subprocess.run([*BUILD, "-o", str(out), str(SRC)], check=True)
    return out


def test_tile_deal_under_sanitizer(exe):
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=ENV)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"


def test_tile_deal_equals_distributed_py(exe):
    p = subprocess.run([str(exe), "cases"], capture_output=True, text=True, timeout=300, env=ENV)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    deals = {}  # (H, T, world, root) -> [slot rows, every rank's tiles]
    for line in p.stdout.splitlines():
        words = line.split()
        if words[0] == "case":
            case = tuple(int(w) for w in words[1:5])
            deals[case] = [int(words[6]), []]
        else:
            assert words[0] == "rank" and words[1] == f"{len(deals[case][1])}:", (case, line)
            deals[case][1].append([int(w) for w in words[2:]])
    assert len(deals) == 15
    for (h, t, world, root), (slot, tiles) in deals.items():
        assert tiles == [rd.rank_tiles(h, r, world, t, root) for r in range(world)], (h, t, world, root)
        assert slot == rd.root_slot_rows(h, world, t, root), (h, t, world, root)
        if root == 1:
            assert slot == rd.slot_rows(h, world, t), (h, t, world, root)
