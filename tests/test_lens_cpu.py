"""The thin lens on the CPU (no GPU needed).

1. tests/native/lens_test.cpp against the shared header raingun_amd/csrc/rg_lens.h (a stand-alone program,
   AddressSanitizer + UBSan, run as a child process): the hash, hand-computed rays, "no lens".
2. The lens reference (rgl_render of tests/native/ref_frames.c through tests/lens_ref.py) tied to the camera reference,
   and through it to the pinned oracle: with an all-zero points table and focus 1 it gives rgc_render's
   bytes and counts at (kW, kH), for the identity camera and a general pose, on test1 and synth64.
3. rg_lens_tables (pure host code of the library): the facts of include/raingun.h.
4. Blur grows with the aperture, on the reference alone.
5. cli.py's --aperture / --focus, Lens, and the lens translation units in every diagnostic build.
"""
import re
import shutil
import subprocess
from pathlib import Path

import ctypes as C
import numpy as np
import pytest

import camera_ref
import lens_ref
import ref_lib
from raingun_amd import _abi, aa
from raingun_amd.camera import Camera, Lens, lens_from_flags
from raingun_amd.cli import parse_arguments
from raingun_amd.scene import SceneDesc
from raingun_amd.synth import synthetic_scene

REPO = Path(__file__).resolve().parents[1]
LOOK = Camera.look_at((3, 2, -10), (0, 0, -30))


# ---------------------------------------------------------------- 1. the shared header
@pytest.fixture(scope="module")
def lens_test_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("lens_test") / "lens_test"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", str(exe),
                    str(REPO / "tests" / "native" / "lens_test.cpp")], check=True, timeout=300)
    return exe


def test_lens_header(lens_test_exe):
    p = subprocess.run([str(lens_test_exe)], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"})
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"


# ---------------------------------------------------------------- 2. the lens reference against the camera reference
def _scene(example_scenes, name):
    return synthetic_scene(64, 8, 8) if name == "synth64" else example_scenes[name]


@pytest.mark.parametrize("pose", ["identity", "look"])
@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_zero_points_table_is_the_camera_reference(example_scenes, name, pose):
    desc = SceneDesc(_scene(example_scenes, name))
    cam = camera_ref.IDENTITY if pose == "identity" else LOOK
    for w, h, k in ((20, 15, 2), (11, 7, 3)):
        zeros = np.zeros((k * k, 2))
        st, rgba, rgb, counts, err = lens_ref.render_samples(desc, cam, Lens(0.75, 1.0), w, h, k, points=zeros)
        c_st, c_rgba, c_rgb, c_counts, c_err = camera_ref.render(desc, cam, k * w, k * h)
        assert (st, err) == (c_st, c_err) == (0, -1), (name, pose, w, h, k)
        assert counts == c_counts, (name, pose, w, h, k, counts, c_counts)
        assert np.array_equal(rgba, c_rgba), (name, pose, w, h, k)
        assert np.array_equal(rgb.view(np.uint32), c_rgb.view(np.uint32)), (name, pose, w, h, k)
    # the control: the real table gives another frame
    st, rgba, _, _, _ = lens_ref.render_samples(desc, cam, Lens(0.75, 1.0), 20, 15, 2)
    assert st == 0 and not np.array_equal(rgba, camera_ref.render(desc, cam, 40, 30)[1])


def test_lens_oracle_is_the_oracle_plus_one_function():
    text = ref_lib.SRC.read_text()
    assert text.count("#include") == 1 and '#include "../../oracle/raingun_oracle.c"' in text
    # one exported function per entry, and one of them the lens's
    assert sorted(re.findall(r"^int32_t (rg\w+)\(", text, re.M)) == ["rga_render", "rgc_render", "rgl_render"]
    for p in (REPO / "raingun_amd").rglob("*"):  # nothing of the product includes or loads it
        if p.is_file() and p.suffix in (".py", ".h", ".hip", ".cpp", ".c") or p.name == "Makefile":
            text = p.read_text(errors="replace")
            assert "ref_frames" not in text and "ref_lib" not in text and "lens_oracle" not in text, p


# ---------------------------------------------------------------- 3. rg_lens_tables
def test_lens_tables():
    points, rot = lens_ref.tables(1)
    assert points.tolist() == [[0.0, 0.0]]
    assert np.all(np.abs((rot ** 2).sum(axis=1) - 1.0) <= 1e-15)
    m = np.arange(64)
    assert np.allclose(rot[:, 0], np.cos(2 * np.pi * m / 64), atol=1e-15) and np.allclose(rot[:, 1], np.sin(2 * np.pi * m / 64), atol=1e-15)
    assert rot[0].tolist() == [1.0, 0.0]
    total = 0
    for k in range(1, 9):
        points, rot_k = lens_ref.tables(k)
        total += len(points)
        assert np.array_equal(rot_k, rot)
        assert np.all((points ** 2).sum(axis=1) <= 1.0), k
        assert len({tuple(p) for p in points.tolist()}) == k * k, k  # pairwise distinct
        if k % 2:
            assert points[(k // 2) * k + k // 2].tolist() == [0.0, 0.0], k
        # a quarter turn maps the set onto itself: (x, y) -> (-y, x) is the point of cell (k - 1 - j, i)
        grid = points.reshape(k, k, 2)  # [j, i]
        turned = np.stack([-grid[..., 1], grid[..., 0]], axis=-1)
        want = np.array([[grid[i, k - 1 - j] for i in range(k)] for j in range(k)])
        assert float(np.abs(turned - want).max()) <= 1e-15, k
        # the centres of the cells, mapped: the first cell lies in the third quadrant, on the diagonal
        if k > 1:
            assert points[0][0] < 0 and abs(points[0][0] - points[0][1]) <= 1e-15
    assert total == 204
    lib = _abi.lib()
    buf = (C.c_double * 128)()
    for bad in (0, 9, 0xFFFFFFFF):
        assert lib.rg_lens_tables(bad, buf, buf) == _abi.RG_ERR_INVALID_ARGUMENT
    assert lib.rg_lens_tables(2, None, buf) == _abi.RG_ERR_INVALID_ARGUMENT
    assert lib.rg_lens_tables(2, buf, None) == _abi.RG_OK  # rotations are optional


# ---------------------------------------------------------------- 4. blur grows with the aperture
def test_blur_grows_with_the_aperture():
    """synthetic_scene(16, 2, 5) at 40x30, k = 2, the reference's view, focus 40 (in front of the spheres, which
    lie 60 to 85 away): the output pixels whose bytes differ from the pinhole supersampled frame number
    0 < n(0.05) < n(1.0) -- 24 and 184 of 1200 in the reference."""
    desc = SceneDesc(synthetic_scene(16, 2, 5))
    w, h, k = 40, 30, 2
    _, _, rgb, _, _ = camera_ref.render(desc, camera_ref.IDENTITY, k * w, k * h)
    _, pinhole = aa.resolve_box(rgb, k)
    n = []
    for aperture in (0.05, 1.0):
        st, rgba, _, counts, err = lens_ref.render(desc, None, Lens(aperture, 40.0), w, h, k)
        assert st == 0 and err == -1 and counts["primary"] == k * k * w * h
        n.append(int(np.count_nonzero((rgba != pinhole).any(axis=2))))
    assert 0 < n[0] < n[1], n


# ---------------------------------------------------------------- 5. flags, Lens, translation units
def test_cli_lens_flags():
    assert parse_arguments(["file"]).lens is None
    o = parse_arguments(["--samples", "3", "--aperture", "0.5", "--focus", "30", "file"])
    assert o.lens == Lens(0.5, 30.0) and o.samples == 3
    o = parse_arguments(["--samples=2", "--aperture=0", "--focus=1e1", "--eye", "3,2,-10", "--look-at", "0,0,-30", "--hd", "file"])
    assert o.lens == Lens(0.0, 10.0) and o.camera == LOOK and (o.width, o.height) == (1920, 1080)


@pytest.mark.parametrize("args", [
    ["--aperture", "0.5"], ["--focus", "3"], ["--samples", "2", "--aperture", "0.5"],
    ["--aperture", "0.5", "--focus", "3"], ["--samples", "1", "--aperture", "0.5", "--focus", "3"],
    ["--samples", "2", "--adaptive", "32", "--aperture", "0.5", "--focus", "3"],
    ["--samples", "2", "--aperture", "-1", "--focus", "3"], ["--samples", "2", "--aperture", "1", "--focus", "0"],
    ["--samples", "2", "--aperture", "x", "--focus", "3"], ["--samples", "2", "--aperture", "1", "--focus", "inf"],
])
def test_cli_lens_flag_errors(args):
    with pytest.raises(SystemExit, match="Could not build the lens") as e:  # as "Could not build the camera"
        parse_arguments([*args, "file"])
    assert isinstance(e.value.code, str)


def test_lens_class():
    assert Lens(1, 2) == Lens(1.0, 2.0) and lens_from_flags(None, None, 1, None) is None
    for bad in ((-1.0, 1.0), (1.0, 0.0), (1.0, -1.0), (float("nan"), 1.0), (1.0, float("inf"))):
        with pytest.raises(ValueError):
            Lens(*bad)


HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_lens_cfg(tmp_path):
    """tests/native/lens_cfg_test.cpp: what RenderCfg decodes from MAXD = -2, compiled as tests/test_camera_cpu.py
    compiles its program (host side only, AddressSanitizer + UBSan)."""
    exe = tmp_path / "lens_cfg_test"
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    str(REPO / "tests" / "native" / "lens_cfg_test.cpp")], check=True, timeout=600)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"})
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_lens_units_compile_in_every_diagnostic_build():
    """The lens units take the kernel headers through rg_lens_launch.h, so tests/test_diagnostic_builds.py does
    not see them: the default build and every diagnostic switch, here."""
    csrc = REPO / "raingun_amd" / "csrc"
    units = sorted(p.name for p in csrc.glob("rg_render_*lens*.hip"))
    assert units == ["rg_render_heavy_lens.hip", "rg_render_light_lens.hip"]
    for u in units:
        assert '#include "rg_lens_launch.h"' in (csrc / u).read_text() and u in (csrc / "Makefile").read_text()
    cmd = [HIPCC, "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fsyntax-only", "-Werror=return-type"]
    flags = ["", "-DRG_TILE_TIMES", "-DRG_WAVE_TIMES", "-DRG_ITER_STATS", "-DRG_BVH_STATS", "-DRG_REGION_STATS"]
    procs = [(u, f, subprocess.Popen(cmd + ([f] if f else []) + [u], cwd=csrc, stdout=subprocess.DEVNULL,
                                     stderr=subprocess.PIPE, text=True)) for f in flags for u in units]
    for u, f, p in procs:
        err = p.communicate(timeout=900)[1]
        assert p.returncode == 0 and " error:" not in err, (u, f, err[-3000:])
