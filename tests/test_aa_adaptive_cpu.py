"""Adaptive anti-aliasing without a GPU: the numpy restatement (raingun_amd.aa.edge_mask,
resolve_adaptive), the sample-tile arithmetic (raingun_amd/csrc/rg_sample_tiles.h, a
stand-alone native program under ASan + UBSan) and the `--adaptive` flag of both command
lines (argument handling only: no render)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from raingun_amd import _abi, _host, aa
from raingun_amd.cli import parse_arguments

REPO = Path(__file__).resolve().parents[1]


# ---------------------------------------------------------------- edge_mask
def _random_rgba(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 4), dtype=np.uint8)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 2), (3, 5), (9, 14)])
def test_threshold_limits(h, w):
    rgba = _random_rgba(h, w, seed=h * 100 + w)
    m0 = aa.edge_mask(rgba, 0)
    assert m0.shape == (h, w) and m0.dtype == np.uint8 and (m0 == 1).all()  # 0 >= 0 even without neighbours
    assert (aa.edge_mask(rgba, 256) == 0).all()                             # a byte difference is at most 255
    flat = np.full((h, w, 4), 90, np.uint8)
    assert (aa.edge_mask(flat, 1) == 0).all()
    for t in (-1, 257):
        with pytest.raises(ValueError):
            aa.edge_mask(rgba, t)


def test_planted_edge_flags_both_sides_at_exactly_t():
    t = 40
    rgba = np.full((6, 8, 4), 100, np.uint8)
    rgba[:, 4:, 1] = 100 + t  # a vertical edge between columns 3 and 4, green only
    m = aa.edge_mask(rgba, t)
    want = np.zeros((6, 8), np.uint8)
    want[:, 3:5] = 1  # both sides: the relation is symmetric
    assert np.array_equal(m, want)
    assert (aa.edge_mask(rgba, t + 1) == 0).all()  # a difference of T - 1 does not flag
    rgba[:, 4:, 1] = 100 - t                       # the sign does not matter
    assert np.array_equal(aa.edge_mask(rgba, t), want)
    # a diagonal neighbour alone is enough
    one = np.full((5, 5, 4), 10, np.uint8)
    one[2, 2, 2] = 10 + t
    assert np.array_equal(aa.edge_mask(one, t), np.pad(np.ones((3, 3), np.uint8), 1))


def test_alpha_is_ignored():
    rgba = np.full((4, 4, 4), 7, np.uint8)
    rgba[..., 3] = _random_rgba(4, 4, 3)[..., 3]
    assert (aa.edge_mask(rgba, 1) == 0).all()


def test_hand_written_4x3():
    # red channel; green and blue constant.  Threshold 10.
    red = np.array([[0, 0, 0, 50],
                    [0, 9, 0, 50],
                    [0, 0, 0, 41]], np.uint8)
    rgba = np.zeros((3, 4, 4), np.uint8)
    rgba[..., 0] = red
    rgba[..., 3] = 255
    # column 3 differs from column 2 by >= 41; (1, 1) differs from its neighbours by 9 only;
    # 50 against 41 is 9.  So columns 2 and 3 are flagged, columns 0 and 1 are not.
    want = np.array([[0, 0, 1, 1],
                     [0, 0, 1, 1],
                     [0, 0, 1, 1]], np.uint8)
    assert np.array_equal(aa.edge_mask(rgba, 10), want)
    # at threshold 9 the 9s count: every pixel has a neighbour 9 or more away
    assert (aa.edge_mask(rgba, 9) == 1).all()
    # at threshold 42 only the 50s against the 0s
    want42 = np.array([[0, 0, 1, 1],
                       [0, 0, 1, 1],
                       [0, 0, 1, 0]], np.uint8)
    assert np.array_equal(aa.edge_mask(rgba, 42), want42)


def test_mask_matches_a_per_pixel_loop():
    rgba = _random_rgba(7, 9, seed=11)
    rgba[2:5, 3:7] = rgba[2, 3]  # a flat patch
    for t in (1, 32, 128, 255):
        want = np.zeros((7, 9), np.uint8)
        for y in range(7):
            for x in range(9):
                m = 0
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if (dy or dx) and 0 <= y + dy < 7 and 0 <= x + dx < 9:
                            m = max(m, int(np.abs(rgba[y, x, :3].astype(int) - rgba[y + dy, x + dx, :3].astype(int)).max()))
                want[y, x] = m >= t
        assert np.array_equal(aa.edge_mask(rgba, t), want)


# ---------------------------------------------------------------- resolve_adaptive
def _frames(h, w, k, seed):
    rng = np.random.default_rng(seed)
    base_rgb = rng.uniform(-0.2, 1.2, size=(h, w, 3)).astype(np.float32)
    base_rgb[:, : w // 2] = np.float32(0.5)  # a flat half: no contrast there
    base_rgb[0, 0] = [np.nan, -1.0, 2.0]
    base_rgb[0, 1] = base_rgb[1, 0] = base_rgb[1, 1] = [0.0, 0.0, 1.0]  # ... around a corner of specials
    base_rgba = np.empty((h, w, 4), np.uint8)
    base_rgba[..., :3] = aa.f32_to_u8(aa.clamp_sample(base_rgb) * np.float32(255.0))
    base_rgba[..., 3] = 255
    samples = rng.uniform(-0.2, 1.2, size=(k * h, k * w, 3)).astype(np.float32)
    return base_rgba, base_rgb, samples


@pytest.mark.parametrize("k", [2, 3])
def test_resolve_adaptive_limits(k):
    base_rgba, base_rgb, samples = _frames(6, 10, k, seed=k)
    box_mean, box_rgba = aa.resolve_box(samples, k)
    mean, rgba, mask = aa.resolve_adaptive(base_rgba, base_rgb, samples, k, 0)
    assert (mask == 1).all() and np.array_equal(rgba, box_rgba)
    assert np.array_equal(mean.view(np.uint32), box_mean.view(np.uint32))
    mean, rgba, mask = aa.resolve_adaptive(base_rgba, base_rgb, samples, k, 256)
    assert (mask == 0).all() and np.array_equal(rgba, base_rgba)
    assert np.array_equal(mean.view(np.uint32), aa.clamp_sample(base_rgb).view(np.uint32))
    # in between: each pixel from the source its mask bit names
    mean, rgba, mask = aa.resolve_adaptive(base_rgba, base_rgb, samples, k, 100)
    assert np.array_equal(mask, aa.edge_mask(base_rgba, 100)) and 0 < mask.sum() < mask.size
    f = mask.astype(bool)
    assert np.array_equal(rgba[f], box_rgba[f]) and np.array_equal(rgba[~f], base_rgba[~f])
    assert np.array_equal(mean[f].view(np.uint32), box_mean[f].view(np.uint32))
    assert np.array_equal(mean[~f].view(np.uint32), aa.clamp_sample(base_rgb)[~f].view(np.uint32))


@pytest.mark.parametrize("t", [0, 1, 32, 255, 256])
def test_resolve_adaptive_one_sample_is_the_base(t):
    base_rgba, base_rgb, _ = _frames(5, 7, 1, seed=9)
    mean, rgba, mask = aa.resolve_adaptive(base_rgba, base_rgb, base_rgb, 1, t)  # k = 1: the samples are the base
    assert np.array_equal(rgba, base_rgba)
    assert np.array_equal(mean.view(np.uint32), aa.clamp_sample(base_rgb).view(np.uint32))
    assert np.array_equal(mask, aa.edge_mask(base_rgba, t))


# ---------------------------------------------------------------- the tile arithmetic
def test_sample_tiles_under_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = tmp_path / "sample_tiles_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(exe), str(REPO / "tests" / "native" / "sample_tiles_test.cpp")], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1",
                            "PATH": "/usr/bin:/bin"})
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"


# ---------------------------------------------------------------- the command lines
def test_python_cli_adaptive_flag():
    assert parse_arguments(["file"]).adaptive is None
    o = parse_arguments(["--samples", "4", "--adaptive", "32", "file"])
    assert (o.samples, o.adaptive) == (4, 32)
    assert parse_arguments(["--adaptive", "0", "file"]).adaptive == 0
    assert parse_arguments(["--adaptive", "256", "file"]).adaptive == 256
    o = parse_arguments(["--samples", "1", "--adaptive", "32", "file"])  # accepted; no effect on the render
    assert (o.samples, o.adaptive) == (1, 32)
    with pytest.raises(SystemExit) as ei:
        parse_arguments(["--adaptive", "257", "file"])
    assert "adaptive must be between 0 and 256" in str(ei.value)
    with pytest.raises(SystemExit) as ei:
        parse_arguments(["--adaptive", "x", "file"])
    assert "Could not parse adaptive" in str(ei.value)


@pytest.fixture(scope="module")
def native_cli():
    if not (_abi.PKG_DIR / "libraingun_hip.so").exists():
        subprocess.run(["make", "-s", "-C", str(_abi.PKG_DIR / "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", str(_host.SRC_DIR)], check=True)
    return str(_host.CLI_PATH)


def test_native_cli_adaptive_flag(native_cli, tmp_path):
    def run(*args):
        return subprocess.run([native_cli, *args], capture_output=True, text=True, timeout=120)

    missing = str(tmp_path / "missing.yml")
    r = run("--help")
    assert r.returncode == 0 and "--adaptive <T>" in r.stdout
    r = run("--samples", "2", "--adaptive", "257", missing)
    assert r.returncode == 1 and "--adaptive <T>" in r.stderr and "257 is not between 0 and 256" in r.stderr
    assert "USAGE" in r.stderr and "For more information try --help" in r.stderr  # clap-style, as --samples
    r = run("--adaptive", "x", missing)
    assert r.returncode == 101 and "Could not parse adaptive" in r.stderr
    r = run("--adaptive")
    assert r.returncode == 1 and "requires a value" in r.stderr
    # in range, and with --samples 1: accepted (the run gets as far as opening the scene file)
    for args in (["--samples", "4", "--adaptive", "32"], ["--samples", "1", "--adaptive=32"], ["--adaptive", "256"]):
        r = run(*args, missing)
        assert r.returncode == 101 and "Could not open input file" in r.stderr


# ---------------------------------------------------------------- the sparse translation units
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_sparse_units_compile_in_every_diagnostic_build():
    """tests/test_diagnostic_builds.py for the two translation units of the SPARSE instantiations, which
    include the kernel headers through rg_sparse_launch.h: the default build and every diagnostic switch."""
    csrc = REPO / "raingun_amd" / "csrc"
    units = ["rg_render_light_sparse.hip", "rg_render_heavy_sparse.hip"]
    for u in units:
        assert '#include "rg_sparse_launch.h"' in (csrc / u).read_text()
    cmd = [HIPCC, "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fsyntax-only", "-Werror=return-type"]
    flags = ["", "-DRG_TILE_TIMES", "-DRG_WAVE_TIMES", "-DRG_ITER_STATS", "-DRG_BVH_STATS", "-DRG_REGION_STATS"]
    procs = [(u, f, subprocess.Popen(cmd + ([f] if f else []) + [u], cwd=csrc, stdout=subprocess.DEVNULL,
                                     stderr=subprocess.PIPE, text=True)) for f in flags for u in units]
    for u, f, p in procs:
        err = p.communicate(timeout=900)[1]
        assert p.returncode == 0 and " error:" not in err, (u, f, err[-3000:])
