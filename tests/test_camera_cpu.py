"""The movable camera on the CPU (no GPU needed).

1. tests/native/camera_test.cpp against the shared header raingun_amd/csrc/rg_camera.h (a stand-alone
   program, AddressSanitizer + UBSan, run as a child process).
2. The camera reference (rgc_render of tests/native/ref_frames.c through tests/camera_ref.py), and with
   it the one pixel loop of that file, tied to the pinned oracle: (a) with the identity camera it gives oracle.render's bytes, ray counts and status; (b) with
   the camera turned 180 degrees about y it gives, on the scene mirrored in x and z, oracle.render's
   frame of the ORIGINAL scene -- untextured scenes only (sphere atan2 texture coordinates and the
   planes' world-axis texture frames do not turn with the scene); and the control: the turned camera
   on the un-mirrored scene differs.
3. cli.py's --eye / --look-at / --up, and Camera.look_at against the native one, bit for bit.
4. The camera translation units (the four of the render kernels, the tile-order probe's) compile in
   the default and in every diagnostic build (tests/test_diagnostic_builds.py does not see them:
   they include the kernel headers through rg_camera_launch.h and rg_tile_probe.h).
"""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import camera_ref
import ref_lib
from raingun_amd.camera import Camera, camera_from_flags, parse_triple
from raingun_amd.cli import parse_arguments
from raingun_amd.scene import SceneDesc
from raingun_amd.synth import synthetic_scene

REPO = Path(__file__).resolve().parents[1]
SIZES = [(64, 48), (17, 3), (97, 61), (1, 1)]
SYNTH = {"synth16p2d5": (16, 2, 5), "synth64p3d8": (64, 3, 8), "synth64p8d5": (64, 8, 5), "synth16p8d8": (16, 8, 8)}
UNTEXTURED = [*SYNTH, "test2"]
ALL = [*UNTEXTURED, "test1", "test3"]

_SCENES = {}


def _scene(example_scenes, name):
    if name not in _SCENES:
        _SCENES[name] = synthetic_scene(*SYNTH[name]) if name in SYNTH else example_scenes[name]
    return _SCENES[name]


# ---------------------------------------------------------------- 1. the shared header
@pytest.fixture(scope="module")
def camera_test_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("camera_test") / "camera_test"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", str(exe),
                    str(REPO / "tests" / "native" / "camera_test.cpp")], check=True, timeout=300)
    return exe


def _run(exe, *args):
    return subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=300,
                          env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1",
                               "PATH": "/usr/bin:/bin"})


def test_camera_header(camera_test_exe):
    p = _run(camera_test_exe)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"


# ---------------------------------------------------------------- 2. the camera reference against the oracle
@pytest.mark.parametrize("name", ALL)
def test_identity_camera_is_the_oracle(oracle_lib, example_scenes, name):
    """Fact (a)."""
    scene = _scene(example_scenes, name)
    desc = SceneDesc(scene)
    for w, h in SIZES:
        o_st, o_rgba, o_rgb, o_counts, o_err = oracle_lib.render(desc, w, h, want_rgb=True)
        st, rgba, rgb, counts, err = camera_ref.render(desc, camera_ref.IDENTITY, w, h)
        assert (st, err) == (o_st, o_err), (name, w, h)
        assert counts == o_counts, (name, w, h, counts, o_counts)
        assert np.array_equal(rgba, o_rgba), (name, w, h)
        assert np.array_equal(rgb.view(np.uint32), o_rgb.view(np.uint32)), (name, w, h)
    # a tiling, padding rows included
    o = oracle_lib.render(desc, 97, 61, tile_rows=8, stride=3, offset=1, want_rgb=True)
    c = camera_ref.render(desc, camera_ref.IDENTITY, 97, 61, tile_rows=8, stride=3, offset=1)
    assert c[0] == o[0] and c[3] == o[3] and c[4] == o[4] and np.array_equal(c[1], o[1])


@pytest.mark.parametrize("name", UNTEXTURED)
def test_turned_camera_on_the_mirrored_scene_is_the_oracle(oracle_lib, example_scenes, name):
    """Fact (b), and the control."""
    scene = _scene(example_scenes, name)
    mirrored = SceneDesc(camera_ref.mirrored_xz(scene))
    desc = SceneDesc(scene)
    for w, h in SIZES:
        o_st, o_rgba, o_rgb, o_counts, o_err = oracle_lib.render(desc, w, h, want_rgb=True)
        st, rgba, rgb, counts, err = camera_ref.render(mirrored, camera_ref.TURNED, w, h)
        assert (st, err) == (o_st, o_err), (name, w, h)
        assert counts == o_counts, (name, w, h, counts, o_counts)
        assert np.array_equal(rgba, o_rgba), (name, w, h, int(np.count_nonzero((rgba != o_rgba).any(axis=2))))
        assert np.array_equal(rgb.view(np.uint32), o_rgb.view(np.uint32)), (name, w, h)
    if name in SYNTH:  # the control: the scene lies behind a camera that was turned alone
        _, o_rgba, _, o_counts, _ = oracle_lib.render(desc, 64, 48)
        _, rgba, _, counts, _ = camera_ref.render(desc, camera_ref.TURNED, 64, 48)
        assert not np.array_equal(rgba, o_rgba) and counts != o_counts


def test_camera_oracle_is_the_oracle_plus_one_function():
    text = ref_lib.SRC.read_text()
    assert text.count("#include") == 1 and '#include "../../oracle/raingun_oracle.c"' in text
    cc, flags = ref_lib.oracle_flags()
    assert all(f in flags for f in ref_lib.REQUIRED_FLAGS)
    # nothing of the product includes or loads it
    for p in (REPO / "raingun_amd").rglob("*"):
        if p.is_file() and p.suffix in (".py", ".h", ".hip", ".cpp", ".c") or p.name == "Makefile":
            text = p.read_text(errors="replace")
            assert "ref_frames" not in text and "ref_lib" not in text and "camera_oracle" not in text, p


# ---------------------------------------------------------------- 3. flags and look_at
def test_cli_camera_flags():
    assert parse_arguments(["file"]).camera is None
    o = parse_arguments(["--eye", "1,2.5,-3e1", "file"])
    assert o.camera == Camera(eye=(1.0, 2.5, -30.0)) and o.camera.forward == (0.0, 0.0, -1.0)
    o = parse_arguments(["--eye", "-1,2,3", "--look-at", "0,0,-30", "file"])  # a leading minus sign
    assert o.camera == Camera.look_at((-1, 2, 3), (0, 0, -30), (0, 1, 0))
    o = parse_arguments(["--eye=3,2,-10", "--look-at=0,0,-30", "--up", "0,0,-1", "--hd", "file"])
    assert o.camera == Camera.look_at((3, 2, -10), (0, 0, -30), (0, 0, -1)) and (o.width, o.height) == (1920, 1080)
    o = parse_arguments(["--look-at", "0,0,-1", "file"])  # from the origin: the reference's view
    assert o.camera == Camera.identity()
    o = parse_arguments(["--draft", "--eye", "0,1,0", "file"])  # --draft leaves the camera alone
    assert o.camera == Camera.at((0, 1, 0)) and (o.width, o.height) == (800, 600)


@pytest.mark.parametrize("args,msg", [
    (["--eye", "1,2"], "Could not parse eye"), (["--eye", "1,2,3,4"], "Could not parse eye"),
    (["--eye", "1,,3"], "Could not parse eye"), (["--eye", "a,b,c"], "Could not parse eye"),
    (["--eye", "1,2,inf"], "Could not parse eye"), (["--look-at", "1;2;3"], "Could not parse look-at"),
    (["--look-at", "0,0,-1", "--up", "nan,0,0"], "Could not parse up"),
    (["--eye", "1,2,3", "--look-at", "1,2,3"], "Could not build the camera"),
    (["--look-at", "0,0,-5", "--up", "0,0,1"], "Could not build the camera"),
    (["--up", "0,1,0"], "Could not build the camera"),
])
def test_cli_camera_flag_errors(args, msg):
    with pytest.raises(SystemExit, match=msg) as e:  # as "Could not parse width": a message, exit status 1
        parse_arguments([*args, "file"])
    assert isinstance(e.value.code, str)


def test_parse_triple_and_flags():
    assert parse_triple("1,2,3") == (1.0, 2.0, 3.0) and parse_triple(" 1 , -2.5,3e2") == (1.0, -2.5, 300.0)
    for bad in ("", "1,2", "1,2,3,", "x,1,2", "1,2,nan", "1 2 3"):
        with pytest.raises(ValueError):
            parse_triple(bad)
    assert camera_from_flags(None, None, None) is None
    with pytest.raises(ValueError):
        Camera(forward=(0.0, -0.0, 0.0))
    with pytest.raises(ValueError):
        Camera(eye=(float("inf"), 0, 0))


POSES = [((3, 2, -10), (0, 0, -30), (0, 1, 0)), ((0, 25, -40), (0, 0, -40), (0, 0, -1)),
         ((-7.5, 1.25, 4), (2, 0.5, -60), (0, 1, 0)), ((1e6, 2e6, -3e6), (0, 0, -30), (0, 1, 0)),
         ((0, 0, 0), (1, 1, 1), (0.3, 1, -0.2)), ((0.1, 0.2, 0.3), (1e-3, 7, -1e5), (1, 0, 0)),
         ((0, 0, 0), (0, 0, -1), (0, 1, 0))]


def test_python_look_at_is_the_native_one(camera_test_exe):
    for eye, target, up in POSES:
        p = _run(camera_test_exe, "look_at", *(float(v).hex() for v in (*eye, *target, *up)))
        assert p.returncode == 0, p.stderr[-2000:]
        native = tuple(float.fromhex(t) for t in p.stdout.split())
        cam = Camera.look_at(eye, target, up)
        ours = (*cam.right, *cam.up, *cam.forward)
        assert [v.hex() for v in ours] == [v.hex() for v in native], (eye, target, up)
    for eye, target, up in [((1, 2, 3), (1, 2, 3), (0, 1, 0)), ((0, 0, 0), (0, 0, -5), (0, 0, 2)),
                            ((0, 0, 0), (0, 0, -5), (0, 0, 0)), ((0, 0, 0), (1e308, -1e308, 1e308), (0, 1, 0))]:
        p = _run(camera_test_exe, "look_at", *(float(v).hex() for v in (*eye, *target, *up)))
        assert p.stdout.strip() == "rejected", (eye, target, up, p.stdout)
        with pytest.raises(ValueError):
            Camera.look_at(eye, target, up)


# ---------------------------------------------------------------- 4. the camera translation units
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_camera_cfg(tmp_path):
    """tests/native/camera_cfg_test.cpp: what RenderCfg decodes from MAXD = -1, compiled as
    tests/test_render_cfg.py compiles its program (host side only, AddressSanitizer + UBSan)."""
    exe = tmp_path / "camera_cfg_test"
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    str(REPO / "tests" / "native" / "camera_cfg_test.cpp")], check=True, timeout=600)
    p = _run(exe)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_camera_units_compile_in_every_diagnostic_build():
    csrc = REPO / "raingun_amd" / "csrc"
    units = sorted(p.name for p in csrc.glob("rg_render_*camera*.hip"))
    assert units == ["rg_render_heavy_camera.hip", "rg_render_heavy_camera_sparse.hip", "rg_render_light_camera.hip",
                     "rg_render_light_camera_sparse.hip"]
    for u in units:
        assert '#include "rg_camera_launch.h"' in (csrc / u).read_text()
    units.append("rg_tile_order_camera.hip")
    assert '#include "rg_tile_probe.h"' in (csrc / units[-1]).read_text()
    for u in units:
        assert u in (csrc / "Makefile").read_text()
    cmd = [HIPCC, "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fsyntax-only", "-Werror=return-type"]
    flags = ["", "-DRG_TILE_TIMES", "-DRG_WAVE_TIMES", "-DRG_ITER_STATS", "-DRG_BVH_STATS", "-DRG_REGION_STATS"]
    procs = [(u, f, subprocess.Popen(cmd + ([f] if f else []) + [u], cwd=csrc, stdout=subprocess.DEVNULL,
                                     stderr=subprocess.PIPE, text=True)) for f in flags for u in units]
    for u, f, p in procs:
        err = p.communicate(timeout=900)[1]
        assert p.returncode == 0 and " error:" not in err, (u, f, err[-3000:])
