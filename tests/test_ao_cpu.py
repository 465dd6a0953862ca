"""The ambient occlusion pass on the CPU (no GPU): its tables, two independent restatements of the contract tied
to the pinned oracle, the shared header, the command line and the bindings.

1. rg_ao_tables (pure host code of the library) against numpy: the facts of include/raingun.h.
2. The rays: raingun_amd.ao.directions (numpy f64) agrees bit for bit with the rays tests/native/ao_ref.c traces.
3. The occlusion: those numpy rays, fed to the oracle's rgo_trace, reproduce the reference's `open` counts --
   ao_ref.c (C, on the oracle's static functions) and ao.directions + rgo_trace (numpy, on the oracle's export)
   are two restatements of the contract that share no line.
4. tests/native/ao_test.cpp: raingun_amd/csrc/rg_ao.h as a stand-alone program, built once more with
   AddressSanitizer + UBSan as its own executable.  Nothing is loaded into Python under a sanitizer.
5. The condition on the parity inputs (tests/ao_cases.py), the scene whose occlusion rays raise
   RG_ERR_NAN_DISTANCE, `--ao`'s parsing, the symbol table and the translation unit's diagnostic builds.
"""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ao_cases
import ao_ref
import aov_ref
from raingun_amd import _abi, ao
from raingun_amd.cli import parse_arguments
from raingun_amd.scene import SceneDesc
from raingun_amd.synth import synthetic_scene

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "native" / "ao_test.cpp"
CXXFLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror"]
HIPCC = "/opt/rocm/bin/hipcc"
INF = float("inf")


# ---------------------------------------------------------------- 1. the tables
def test_ao_tables():
    import lens_ref

    eps = np.finfo(np.float64).eps
    for k in range(1, 9):
        p = ao.tables(k)
        disk, _ = lens_ref.tables(k)
        assert p.shape == (k * k, 3)
        assert np.array_equal(aov_ref.bits(p[:, :2]), aov_ref.bits(disk))
        # z as the header states it, in numpy's f64
        z = np.sqrt(np.maximum(0.0, (1.0 - p[:, 0] * p[:, 0]) - p[:, 1] * p[:, 1]))
        assert np.array_equal(aov_ref.bits(p[:, 2]), aov_ref.bits(z)), k
        assert (p[:, 2] >= 0.0).all()
        # unit length: x^2 + y^2 + fl(sqrt(fl(1 - x^2 - y^2)))^2, a handful of roundings of values <= 1
        assert np.abs((p * p).sum(axis=1) - 1.0).max() <= 4 * eps, k
        if k % 2 == 1:
            centre = p[(k // 2) * k + k // 2]
            assert tuple(centre) == (0.0, 0.0, 1.0) and not np.signbit(centre).any()
    assert np.array_equal(ao.tables(1), [[0.0, 0.0, 1.0]])
    rot = ao.rotations()
    assert rot.shape == (64, 2) and tuple(rot[0]) == (1.0, 0.0)


def test_ao_tables_rejections():
    lib = _abi.lib()
    buf = (C.c_double * (3 * 81))()
    for bad in (0, 9, 0xFFFFFFFF):
        assert lib.rg_ao_tables(bad, buf) == _abi.RG_ERR_INVALID_ARGUMENT
    assert lib.rg_ao_tables(2, None) == _abi.RG_ERR_INVALID_ARGUMENT
    assert lib.rg_ao_tables(8, buf) == _abi.RG_OK
    for bad in (0, 9):
        with pytest.raises(ValueError):
            ao.tables(bad)


# ---------------------------------------------------------------- 2, 3. the two restatements
def _restatement_scenes(example_scenes):
    return {"test1": example_scenes["test1"], "synth": synthetic_scene(16, 2, 5)}


@pytest.mark.parametrize("name", ["test1", "synth"])
@pytest.mark.parametrize("k,radius,bias,posed", [(3, INF, 1e-13, False), (2, 8.0, 1e-6, True)])
def test_rays_and_occlusion_restated(oracle_lib, example_scenes, name, k, radius, bias, posed):
    w, h = 17, 3
    scene = _restatement_scenes(example_scenes)[name]
    cam = ao_cases.CLI_CAMERA if posed else None
    st, frame, counts, err, opened, rays = ao_ref.render(scene, w, h, k, radius, bias, cam, want_rays=True)
    assert st == 0 and err == -1
    # the primary hits, from the AOV reference (the pinned oracle's trace and surface_normal)
    st_a, layers, _, _ = aov_ref.render(scene, w, h, cam)
    assert st_a == 0
    body, depth = layers["body"].ravel(), layers["depth"].ravel()
    hit = body >= 0
    assert np.array_equal(hit, opened.ravel() >= 0) and hit.any()
    assert counts == {"primary": w * h, "shadow": k * k * int(hit.sum()), "secondary": 0}
    fa = oracle_lib.lib().rgo_fov_adjustment(scene.fov)
    prime = aov_ref.prime_rays(scene.fov, w, h, fa) if cam is None else _camera_rays(cam, w, h, fa)
    # surface_normal in f64: the AOV layer holds its f32, so restate it from the scene (spheres, planes)
    normal = _normals_f64(scene, body, prime, depth)
    pixel = np.arange(w * h, dtype=np.uint32)
    O, D = ao.directions(prime[hit, :3], prime[hit, 3:], depth[hit], normal[hit], pixel[hit], k, bias)
    got = rays.reshape(w * h, k * k, 6)[hit]
    assert np.array_equal(aov_ref.bits(got[..., :3]), aov_ref.bits(np.broadcast_to(O[:, None, :], got[..., :3].shape)))
    assert np.array_equal(aov_ref.bits(got[..., 3:]), aov_ref.bits(D)), f"{name}: directions differ"
    assert not rays.reshape(w * h, k * k, 6)[~hit].any()
    # 3. the occlusion from the numpy rays and the oracle's exported trace
    mine = np.concatenate([np.broadcast_to(O[:, None, :], D.shape), D], axis=2).reshape(-1, 6)
    t_st, dist, tbody = oracle_lib.trace(SceneDesc(scene), mine)
    assert t_st == 0
    occluded = (tbody >= 0) & ~(dist > radius)
    open_mine = (~occluded).reshape(-1, k * k).sum(axis=1)
    assert np.array_equal(open_mine, opened.ravel()[hit])
    value = open_mine.astype(np.float32) / np.float32(k * k)
    assert np.array_equal(aov_ref.bits(value), aov_ref.bits(frame.ravel()[hit]))
    assert (frame.ravel()[~hit] == 1.0).all()


def _camera_rays(cam, width, height, fov_adjustment):
    """The camera rays of include/raingun.h (rg_camera) in numpy f64, its expression order: (H*W, 6)."""
    x = np.arange(width, dtype=np.float64)[None, :]
    y = np.arange(height, dtype=np.float64)[:, None]
    aspect = np.float64(width) / np.float64(height)
    sx = np.broadcast_to(((((x + 0.5) / np.float64(width)) * 2.0 - 1.0) * aspect) * fov_adjustment, (height, width))
    sy = np.broadcast_to((1.0 - ((y + 0.5) / np.float64(height)) * 2.0) * fov_adjustment, (height, width))
    d = np.stack([(cam.right[c] * sx + cam.up[c] * sy) + cam.forward[c] for c in range(3)], axis=2)
    inv = 1.0 / np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    rays = np.zeros((height, width, 6), dtype=np.float64)
    rays[..., :3] = np.asarray(cam.eye, np.float64)
    rays[..., 3:] = d * inv[..., None]
    return rays.reshape(-1, 6)


def _normals_f64(scene, body, prime, depth):
    """surface_normal (bodies.rs) of spheres, planes and disks in numpy f64, per pixel; zeros on a miss."""
    from raingun_amd.scene import Disk, Plane, Sphere

    with np.errstate(invalid="ignore"):
        hitp = prime[:, :3] + prime[:, 3:] * depth[:, None]
    n = np.zeros((body.size, 3))
    for i, b in enumerate(scene.bodies):
        sel = body == i
        if not sel.any():
            continue
        if isinstance(b, Sphere):
            v = hitp[sel] - np.asarray(b.center, np.float64)
            inv = 1.0 / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            n[sel] = v * inv[:, None]
        elif isinstance(b, (Plane, Disk)):
            n[sel] = -np.asarray(b.normal, np.float64)
        else:
            pytest.fail(f"no f64 normal stated here for {type(b).__name__}")
    return n


# ---------------------------------------------------------------- 4. the shared header
def _cxx():
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    return cxx


def test_ao_header(tmp_path):
    exe = tmp_path / "ao_test"
    subprocess.run([_cxx(), *CXXFLAGS, "-o", str(exe), str(SRC)], check=True, timeout=300)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"


def test_ao_header_sanitized(tmp_path):
    """The same program as its own executable under AddressSanitizer + UBSan."""
    exe = tmp_path / "ao_test_san"
    subprocess.run([_cxx(), *CXXFLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), str(SRC)],
                   check=True, timeout=300)
    env = {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"


def test_ao_ref_is_ref_frames_plus_one_entry():
    text = ao_ref.SRC.read_text()
    assert '#include "ref_frames.c"' in text and "rg_ao.h" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    exported = re.findall(r"^(?:int32_t|void|uint32_t|double)\s+(\w+)\(", code, re.M)
    assert exported == ["rgao_render"]


# ---------------------------------------------------------------- 5. inputs, errors, command line, bindings
@pytest.mark.parametrize("name", ao_cases.SCENES)
def test_parity_inputs_meet_the_condition(example_scenes, name):
    ao_cases.assert_condition(example_scenes, name)


def test_closed_room_is_wholly_occluded_at_infinity(example_scenes):
    """Why synth64 runs with two finite radii (tests/ao_cases.py)."""
    st, frame, _, _, opened, _ = ao_cases.ref(example_scenes, "synth64", ao_cases.W, ao_cases.H, 8)
    assert st == 0 and ao_cases.partial_share(frame, opened) < ao_cases.MIN_PARTIAL


def test_identity_camera_and_tilings_on_the_reference(example_scenes):
    import camera_ref

    scene, w, h, k = example_scenes["test1"], 17, 11, 2
    st, whole, counts, _, _, _ = ao_ref.render(scene, w, h, k, 8.0)
    st1, ident, counts1, _, _, _ = ao_ref.render(scene, w, h, k, 8.0, cam=camera_ref.IDENTITY)
    assert st == st1 == 0 and counts == counts1
    assert np.array_equal(aov_ref.bits(whole), aov_ref.bits(ident))
    st2, part, _, _, opened, _ = ao_ref.render(scene, w, h, k, 8.0, tile_rows=4, stride=2, offset=0)
    assert st2 == 0 and part.shape == (8, w)  # tiles 0 (rows 0..3) and 2 (rows 8..10 and one padding row)
    assert np.array_equal(aov_ref.bits(part[:4]), aov_ref.bits(whole[:4]))
    assert np.array_equal(aov_ref.bits(part[4:7]), aov_ref.bits(whole[8:11]))
    assert (part[7] == 0.0).all() and (opened[7] == -1).all()


def test_nan_distance_comes_from_an_occlusion_ray():
    """The scene tests/test_gpu_ao.py relies on: the primary rays alone are answered without an error, the pass
    reports RG_ERR_NAN_DISTANCE, and the frame is delivered."""
    scene, w, h = ao_cases.nan_scene(), 17, 11
    st_a, layers, _, err_a = aov_ref.render(scene, w, h)
    assert st_a == 0 and err_a == -1 and (layers["body"] != 0).all()  # no primary ray meets the far sphere
    st, frame, counts, err, opened, _ = ao_ref.render(scene, w, h, 2)
    assert st == _abi.RG_ERR_NAN_DISTANCE and 0 <= err < w * h
    assert layers["body"].ravel()[err] in (1, 2)  # on the floor or the ceiling: (5e154 d.y)^2 overflows either way
    assert counts == {"primary": w * h, "shadow": 4 * int((layers["body"] >= 0).sum()), "secondary": 0}
    assert np.isfinite(frame).all()


def test_visualize():
    a = np.array([[0.0, 1.0, 0.5, 0.25], [1.0 / 9.0, np.nan, -1.0, 2.0]], np.float32)
    img = ao.visualize(a)
    assert img.shape == (2, 4, 4) and img.dtype == np.uint8 and (img[..., 3] == 255).all()
    assert img[..., 0].tolist() == [[0, 255, 127, 63], [28, 0, 0, 255]]
    assert np.array_equal(img[..., 0], img[..., 1]) and np.array_equal(img[..., 0], img[..., 2])
    with pytest.raises(ValueError):
        ao.visualize(np.zeros((2, 2, 3), np.float32))


def test_cli_ao_flag():
    yml = str(REPO / "tests" / "golden" / "examples" / "test1.yml")
    assert parse_arguments([yml]).ao is None
    assert parse_arguments([yml, "--ao", "4"]).ao == (4, INF, 1e-13)
    assert parse_arguments([yml, "--ao", "3,5.0"]).ao == (3, 5.0, 1e-13)
    assert parse_arguments([yml, "--ao", "2,inf,1e-6"]).ao == (2, INF, 1e-6)
    o = parse_arguments([yml, "--ao", "2", "--samples", "3", "--aov", "depth", "--draft"])
    assert o.ao == (2, INF, 1e-13) and o.samples == 3 and o.aov == ("depth",) and (o.width, o.height) == (800, 600)
    assert ao.parse_spec("8,0.5,0") == (8, 0.5, 0.0)
    for bad in ("", "0", "9", "x", "2,", "2,0", "2,-1", "2,nan", "2,1,-1e-13", "2,1,inf", "2,1,nan", "2,1,0,0", "2.5"):
        with pytest.raises(ValueError):
            ao.parse_spec(bad)
        with pytest.raises(SystemExit, match="Could not parse ao"):
            parse_arguments([yml, "--ao", bad])


def test_rg_ao_layout_and_symbols():
    text = (REPO / "include" / "raingun.h").read_text()
    m = re.search(r"typedef struct rg_ao \{(.*?)\} rg_ao;", text, re.S)
    fields = re.findall(r"^\s*(uint32_t|double)\s+(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S), re.M)
    assert fields == [("uint32_t", "samples"), ("uint32_t", "_pad"), ("double", "radius"), ("double", "bias")]
    assert [f[0] for f in _abi.rg_ao._fields_] == [f[1] for f in fields]
    assert C.sizeof(_abi.rg_ao) == 24 and _abi.rg_ao.radius.offset == 8 and _abi.rg_ao.bias.offset == 16
    assert {"rg_ao_tables", "rg_render_ao", "rg_render_ao_async"} <= set(_abi.EXPORTED_SYMBOLS)
    lib = _abi.lib()
    for sym in ("rg_ao_tables", "rg_render_ao", "rg_render_ao_async"):
        assert getattr(lib, sym) is not None


def test_rejections_without_a_device():
    lib = _abi.lib()
    INVALID = _abi.RG_ERR_INVALID_ARGUMENT
    buf = np.full(16, 7.0, np.float32)
    good = _abi.rg_ao(2, 0, INF, 1e-13)
    t = _abi.rg_tiling(4, 1, 0)
    assert lib.rg_render_ao(None, 4, 4, C.byref(good), buf.ctypes.data, None) == INVALID
    assert lib.rg_render_ao_async(None, 4, 4, C.byref(t), C.byref(good), buf.ctypes.data, None, None) == INVALID
    assert (buf == 7.0).all()


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_ao_unit_compiles_in_every_diagnostic_build():
    """rg_ao.hip takes the kernel headers through rg_ao_kernel.h, so tests/test_diagnostic_builds.py does not see
    it: the default build and every diagnostic switch, here."""
    csrc = REPO / "raingun_amd" / "csrc"
    assert '#include "rg_ao_kernel.h"' in (csrc / "rg_ao.hip").read_text()
    make = (csrc / "Makefile").read_text()
    assert "rg_ao.hip" in make and "rg_ao_kernel.h" in make and "rg_ao.h" in make
    cmd = [HIPCC, "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fsyntax-only", "-Werror=return-type"]
    flags = ["", "-DRG_TILE_TIMES", "-DRG_WAVE_TIMES", "-DRG_ITER_STATS", "-DRG_BVH_STATS", "-DRG_REGION_STATS"]
    procs = [(f, subprocess.Popen(cmd + ([f] if f else []) + ["rg_ao.hip"], cwd=csrc, stdout=subprocess.DEVNULL,
                                  stderr=subprocess.PIPE, text=True)) for f in flags]
    for f, p in procs:
        err = p.communicate(timeout=900)[1]
        assert p.returncode == 0 and " error:" not in err, (f, err[-3000:])
