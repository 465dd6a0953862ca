"""AOV layers on the CPU (no GPU needed): the AOV reference (rga_render of tests/native/ref_frames.c
through tests/aov_ref.py) tied to the pinned oracle, aov.visualize's known answers, and the bindings.

(a) `body` and `depth` of the reference equal rgo_trace on create_prime's rays, bit for bit (a miss is
    -1 / 0.0 there and -1 / +inf here), and the identity camera gives the same layers.
(b) On a scene whose bodies are all diffuse, shading pixels in Python from the reference's `normal` and
    `albedo` layers (shade_diffuse, rendering.rs:132-172, shadow rays through rgo_trace) reproduces
    rgo_render's f32 RGB to 1e-6; and directly: `albedo` of a flat-colour body is its colour, `normal`
    of a plane is -n.
(c) aov.visualize on hand-made arrays.
Also: rg_aov.hip compiles in the default and in every diagnostic build (tests/test_diagnostic_builds.py
does not see it: it takes the kernel headers through rg_aov_kernel.h).
"""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import aov_ref
import camera_ref
from raingun_amd import _abi, aov
from raingun_amd.cli import parse_arguments
from raingun_amd.color import Color
from raingun_amd.scene import (DirectionalLight, Material, Plane, Scene, SceneDesc, Sphere, SphericalLight)
from raingun_amd.synth import synthetic_scene

REPO = Path(__file__).resolve().parents[1]
HIPCC = "/opt/rocm/bin/hipcc"
SIZES = [(97, 61), (160, 120)]
F32 = np.float32
PI_F32 = F32(3.14159265358979323846)


def _scene(example_scenes, name):
    return synthetic_scene(64, 8, 8) if name == "synth64" else example_scenes[name]


# ---------------------------------------------------------------- (a) body and depth against rgo_trace
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ["test1", "test2", "test3", "synth64"])
def test_body_and_depth_are_rgo_trace(oracle_lib, example_scenes, name, w, h):
    scene = _scene(example_scenes, name)
    desc = SceneDesc(scene)
    st, out, counts, err = aov_ref.render(desc, w, h)
    assert st == 0 and err == -1 and counts == {"primary": w * h, "shadow": 0, "secondary": 0}
    rays = aov_ref.prime_rays(scene.fov, w, h, oracle_lib.lib().rgo_fov_adjustment(scene.fov))
    t_st, dist, body = oracle_lib.trace(desc, rays)
    assert t_st == 0
    miss = body < 0
    assert int((~miss).sum()) > 0
    assert np.array_equal(out["body"].ravel(), body)
    want = np.where(miss, np.inf, dist)
    assert np.array_equal(aov_ref.bits(out["depth"].ravel()), aov_ref.bits(want))
    # misses: nothing under the pixel
    assert not out["normal"].reshape(-1, 3)[miss].any() and not out["uv"].reshape(-1, 2)[miss].any()
    dc = scene.default_color
    assert (out["albedo"].reshape(-1, 3)[miss] == np.array([dc.red, dc.green, dc.blue], F32)).all()
    # the identity camera is create_prime
    st1, out1, counts1, err1 = aov_ref.render(desc, w, h, camera_ref.IDENTITY)
    assert (st1, counts1, err1) == (st, counts, err)
    for n in aov.LAYERS:
        assert np.array_equal(aov_ref.bits(out1[n]), aov_ref.bits(out[n])), n


def test_tilings_and_subsets_of_the_reference(example_scenes):
    scene, w, h = example_scenes["test1"], 97, 61
    st, whole, _, _ = aov_ref.render(scene, w, h)
    st2, part, counts, _ = aov_ref.render(scene, w, h, tile_rows=8, stride=3, offset=1)
    assert st == st2 == 0
    rows = [y for t in range(1, 8, 3) for y in range(8 * t, 8 * t + 8)]
    live = [y < h for y in rows]
    assert counts["primary"] == w * sum(live)
    for n in aov.LAYERS:
        assert part[n].shape[0] == len(rows)
        for k, y in enumerate(rows):
            if y < h:
                assert np.array_equal(aov_ref.bits(part[n][k]), aov_ref.bits(whole[n][y])), (n, y)
    pad = [k for k, y in enumerate(rows) if y >= h]
    assert pad and (part["body"][pad] == -1).all() and np.isposinf(part["depth"][pad]).all()
    assert not part["normal"][pad].any() and not part["uv"][pad].any() and not part["albedo"][pad].any()
    st3, only, _, _ = aov_ref.render(scene, w, h, layers=("depth", "uv"))
    assert st3 == 0 and sorted(only) == ["depth", "uv"]
    assert np.array_equal(aov_ref.bits(only["uv"]), aov_ref.bits(whole["uv"]))


# ---------------------------------------------------------------- (b) diffuse reconstruction
def _diffuse_scene():
    red, green, grey = Color.from_str("#d04030"), Color.from_str("#30c060"), Color.from_str("#b0b0b0")
    return Scene(fov=70.0, default_color=Color.from_str("#102030"),
                 bodies=[Plane((0.0, -2.0, 0.0), (0.0, -1.0, 0.0), Material(grey, 0.4)),
                         Sphere((-1.5, -0.5, -7.0), 1.5, Material(red, 0.5)),
                         Sphere((1.8, 0.0, -6.0), 1.0, Material(green, 0.3)),
                         Sphere((0.3, 1.5, -9.0), 1.2, Material(grey, 0.6))],
                 lights=[DirectionalLight((0.4, -1.0, -0.3), Color.from_str("#ffffff"), 1.5),
                         SphericalLight((3.0, 4.0, -3.0), Color.from_str("#ffd0a0"), 900.0)])


def _normalize(v):
    return v * (1.0 / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def test_diffuse_frame_from_normal_and_albedo(oracle_lib):
    scene, w, h = _diffuse_scene(), 64, 48
    desc = SceneDesc(scene)
    o_st, _, o_rgb, _, _ = oracle_lib.render(desc, w, h, want_rgb=True)
    st, out, _, _ = aov_ref.render(desc, w, h)
    assert o_st == st == 0
    rays = aov_ref.prime_rays(scene.fov, w, h, oracle_lib.lib().rgo_fov_adjustment(scene.fov)).reshape(h, w, 6)
    picked = [(y, x) for y in range(2, h, 7) for x in range(3, w, 9)]
    assert len(picked) >= 36
    hits = 0
    for y, x in picked:
        b = int(out["body"][y, x])
        if b < 0:
            assert np.array_equal(o_rgb[y, x], out["albedo"][y, x])  # the default colour
            continue
        hits += 1
        n = out["normal"][y, x].astype(np.float64)
        hit = rays[y, x, :3] + rays[y, x, 3:] * out["depth"][y, x]
        body_color = out["albedo"][y, x]
        fin = np.zeros(3, F32)
        for l in scene.lights:  # shade_diffuse, rendering.rs:132-172
            if isinstance(l, DirectionalLight):
                dl, ldist, inten = _normalize(-np.array(l.direction)), np.inf, F32(l.intensity)
            else:
                v = np.array(l.position) - hit
                dl, ldist = _normalize(v), np.sqrt(_dot(v, v))
                inten = F32(l.intensity) / (F32(4.0) * PI_F32 * F32(_dot(v, v)))
            _, sd, sb = oracle_lib.trace(desc, np.concatenate([hit + n * 1e-13, dl]))
            in_light = sb[0] < 0 or sd[0] > ldist
            power = np.maximum(F32(_dot(n, dl)), F32(0.0)) * (inten if in_light else F32(0.0))
            reflected = F32(scene.bodies[b].material.albedo) / PI_F32
            lc = np.array([l.color.red, l.color.green, l.color.blue], F32) * power * reflected
            fin = fin + body_color * lc
        fin = np.maximum(np.minimum(fin, F32(1.0)), F32(0.0))
        assert float(np.abs(fin.astype(np.float64) - o_rgb[y, x].astype(np.float64)).max()) <= 1e-6, (y, x, fin, o_rgb[y, x])
    assert hits >= 24


def test_flat_colour_and_plane_normal():
    scene, w, h = _diffuse_scene(), 64, 48
    st, out, _, _ = aov_ref.render(scene, w, h)
    assert st == 0
    for i, b in enumerate(scene.bodies):
        sel = out["body"] == i
        assert sel.any(), i
        c = b.material.coloration
        assert (out["albedo"][sel] == np.array([c.red, c.green, c.blue], F32)).all()
    plane = out["body"] == 0
    assert (out["normal"][plane] == np.array([0.0, 1.0, 0.0], F32)).all()  # -n of the plane's (0, -1, 0)
    sph = out["body"] > 0
    length = np.sqrt((out["normal"][sph].astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(length - 1.0).max() < 1e-6


# ---------------------------------------------------------------- (c) the pictures
def test_visualize_known_answers():
    body = np.array([[-1, 0, 41]], np.int32)
    pic = aov.visualize("body", body)
    assert pic.shape == (1, 3, 4) and pic.dtype == np.uint8 and (pic[..., 3] == 255).all()
    assert tuple(pic[0, 0]) == (0, 0, 0, 255)
    assert tuple(pic[0, 1]) == (0x9E, 0x37, 0x79, 255)  # 1 * 2654435761 = 0x9E3779B1
    hsh = (42 * 2654435761) % 2 ** 32
    assert tuple(pic[0, 2, :3]) == (hsh >> 24, (hsh >> 16) & 255, (hsh >> 8) & 255)
    depth = np.array([[np.inf, 2.0, 4.0, 3.0]])
    pic = aov.visualize("depth", depth)
    assert [tuple(p) for p in pic[0]] == [(0, 0, 0, 255), (255, 255, 255, 255), (0, 0, 0, 255), (127, 127, 127, 255)]
    pic = aov.visualize("depth", np.array([[5.0, np.inf, 5.0]]))  # tmin == tmax
    assert [tuple(p[:3]) for p in pic[0]] == [(255, 255, 255), (0, 0, 0), (255, 255, 255)]
    assert not aov.visualize("depth", np.full((2, 2), np.inf))[..., :3].any()  # nothing hit
    normal = np.array([[[0, 0, 0], [0, 1, 0], [-1, 0, 1]]], F32)
    pic = aov.visualize("normal", normal)
    assert [tuple(p[:3]) for p in pic[0]] == [(0, 0, 0), (127, 255, 127), (0, 127, 255)]
    uv = np.array([[[0.25, 0.5], [1.25, -0.25], [-3.0, 7.5]]], F32)  # outside [0, 1): the fractional part
    pic = aov.visualize("uv", uv)
    assert [tuple(p) for p in pic[0]] == [(63, 127, 0, 255), (63, 191, 0, 255), (0, 127, 0, 255)]
    albedo = np.array([[[0.0, 0.5, 1.0], [2.0, -1.0, np.nan]]], F32)
    pic = aov.visualize("albedo", albedo)
    assert [tuple(p[:3]) for p in pic[0]] == [(0, 127, 255), (255, 0, 0)]
    with pytest.raises(ValueError):
        aov.visualize("beauty", body)
    with pytest.raises(ValueError):
        aov.visualize("normal", body)


def test_layer_names():
    assert aov.parse_layers("all") == aov.LAYERS
    assert aov.parse_layers("uv,body") == ("body", "uv")
    assert aov.parse_layers(["depth"]) == ("depth",)
    for bad in ("", "body,", "beauty", "body,colour"):
        with pytest.raises(ValueError):
            aov.parse_layers(bad)
    yml = str(REPO / "tests" / "golden" / "examples" / "test1.yml")
    assert parse_arguments([yml, "--aov", "normal,depth"]).aov == ("depth", "normal")
    assert parse_arguments([yml]).aov == ()
    with pytest.raises(SystemExit):
        parse_arguments([yml, "--aov", "beauty"])


# ---------------------------------------------------------------- header and bindings
def test_rg_aov_layout_matches_the_header():
    text = (REPO / "include" / "raingun.h").read_text()
    m = re.search(r"typedef struct rg_aov \{(.*?)\} rg_aov;", text, re.S)
    fields = re.findall(r"^\s*(int32_t|double|float)\s*\*(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S), re.M)
    assert [f[1] for f in fields] == list(aov.LAYERS) == [f[0] for f in _abi.rg_aov._fields_]
    assert [f[0] for f in fields] == ["int32_t", "double", "float", "float", "float"]
    assert C.sizeof(_abi.rg_aov) == 5 * C.sizeof(C.c_void_p)
    for k, n in enumerate(aov.LAYERS):
        assert getattr(_abi.rg_aov, n).offset == k * C.sizeof(C.c_void_p)
    assert {"rg_render_aov", "rg_render_aov_async"} <= set(_abi.EXPORTED_SYMBOLS)


def test_rejections_without_a_device():
    lib = _abi.lib()
    INVALID = _abi.RG_ERR_INVALID_ARGUMENT
    buf = np.zeros(16, np.float64)
    some = _abi.rg_aov(depth=buf.ctypes.data)
    t = _abi.rg_tiling(4, 1, 0)
    assert lib.rg_render_aov(None, 4, 4, C.byref(some), None) == INVALID
    assert lib.rg_render_aov_async(None, 4, 4, C.byref(t), C.byref(some), None, None) == INVALID
    assert lib.rg_render_aov(None, 4, 4, None, None) == INVALID


# ---------------------------------------------------------------- the translation unit
@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_aov_unit_compiles_in_every_diagnostic_build():
    csrc = REPO / "raingun_amd" / "csrc"
    assert '#include "rg_aov_kernel.h"' in (csrc / "rg_aov.hip").read_text()
    assert "rg_aov.hip" in (csrc / "Makefile").read_text() and "rg_aov_kernel.h" in (csrc / "Makefile").read_text()
    cmd = [HIPCC, "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fsyntax-only", "-Werror=return-type"]
    flags = ["", "-DRG_TILE_TIMES", "-DRG_WAVE_TIMES", "-DRG_ITER_STATS", "-DRG_BVH_STATS", "-DRG_REGION_STATS"]
    procs = [(f, subprocess.Popen(cmd + ([f] if f else []) + ["rg_aov.hip"], cwd=csrc, stdout=subprocess.DEVNULL,
                                  stderr=subprocess.PIPE, text=True)) for f in flags]
    for f, p in procs:
        err = p.communicate(timeout=900)[1]
        assert p.returncode == 0 and " error:" not in err, (f, err[-3000:])
