"""CPU checks of the ambient term (include/raingun.h rg_ao_filter / rg_render_image_ambient), no GPU involved.

1. The numpy restatement (raingun_amd/ambient.py) agrees bit for bit with the C reference (tests/native/ambient_ref.c,
   written from the header's text): filter, shares, compose.  Two restatements that share no line.
2. The conditions on the test inputs (tests/ambient_cases.py), on the reference.
3. tests/native/ambient_test.cpp: raingun_amd/csrc/rg_ambient.h as a stand-alone program, built once more with
   AddressSanitizer + UBSan as its own executable.  Nothing is loaded into Python under a sanitizer.
4. The quality statement: on the reference the filtered frame is closer to a 576-rays-per-pixel truth than the
   unfiltered one at the same k, at k = 2, 3 and 4, on five cases.

   At 160x90 (DESIGN.md 4aa's table was taken at 480x270; ratios filtered / unfiltered RMS error measured here):
       test1 inf    k2 .59  k3 .84  k4 .49        test1 r 8     k2 .76  k3 .68  k4 .74
       test2 inf    k2 .45  k3 .56  k4 .77        open64 inf    k2 .40  k3 .87  k4 .45
       open64 r 24  k2 .58  k3 .60  k4 .69
5. Colour 0 composes to the resolve's bytes, the rejections that need no device, both command lines' parsing, the
   ABI mirror and the translation units' build.
"""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ambient_cases
import ambient_ref
import ao_cases
import ao_ref
import aov_ref
from aov_ref import bits
from raingun_amd import _abi, aa, ambient
from raingun_amd.cli import parse_arguments
from raingun_amd.color import Color
from raingun_amd.scene import Material, Scene, SceneDesc, Sphere

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "native" / "ambient_test.cpp"
CXXFLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror"]
HIPCC = "/opt/rocm/bin/hipcc"
INF = float("inf")
QUALITY_SIZE = (160, 90)
QUALITY_CASES = [("test1", INF), ("test1", 8.0), ("test2", INF), ("open64", INF), ("open64", 24.0)]


# ---------------------------------------------------------------- 1. numpy == C
@pytest.mark.parametrize("w,h", ambient_cases.SIZES)
def test_numpy_filter_is_the_reference(w, h):
    ao, body, normal = ambient_cases.guides(w, h)
    for r in ambient_cases.RADII:
        for nmin in ambient_cases.NORMAL_MINS:
            want = ambient_ref.filter_ao(ao, body, normal, r, nmin)
            got = ambient.filter_ao(ao, body, normal, r, nmin)
            assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), (w, h, r, nmin)
            miss = body < 0
            assert np.array_equal(bits(want)[miss], bits(ao)[miss])
        rev_c = ambient_ref.filter_ao(ao, body, normal, r, 0.9, reverse=True)
        assert np.array_equal(bits(ambient.filter_ao(ao, body, normal, r, 0.9, reverse=True)), bits(rev_c))


def test_numpy_filter_on_a_scene(example_scenes):
    raw, body, normal = ambient_cases.scene_layers(example_scenes, "test1", *ambient_cases.combos("test1")[0])
    for r, nmin in ((1, 1.0), (2, 0.9), (8, 0.0)):
        assert np.array_equal(bits(ambient.filter_ao(raw, body, normal, r, nmin)),
                              bits(ambient_ref.filter_ao(raw, body, normal, r, nmin)))


def test_filter_facts():
    """A constant frame over one flat body stays constant up to rounding of the sum; a lone body pixel keeps its
    value exactly; normal_min 1 still accepts identical normals."""
    h, w = 9, 11
    ao = np.full((h, w), 0.75, np.float32)
    body = np.zeros((h, w), np.int32)
    normal = np.broadcast_to(np.array([0.0, 3.0, 0.0], np.float32), (h, w, 3)).copy()  # not unit
    for r in (1, 2, 8):
        out = ambient_ref.filter_ao(ao, body, normal, r, 1.0)
        assert np.array_equal(out, ao)  # 0.75 w sums exactly
    body2 = np.arange(h * w, dtype=np.int32).reshape(h, w)  # every pixel its own body
    noisy = np.random.default_rng(1).random((h, w), dtype=np.float32)
    out = ambient_ref.filter_ao(noisy, body2, normal, 2, 0.0)
    assert np.array_equal(bits(out), bits((np.float32(9.0) * noisy) / np.float32(9.0)))
    with pytest.raises(ValueError):
        ambient.filter_ao(ao, body, normal, 0, 0.9)
    with pytest.raises(ValueError):
        ambient.filter_ao(ao, body, normal, 2, float("nan"))


def _material(surface, albedo, reflectivity=0.0):
    return Material(Color.from_str("#808080"), albedo, surface=surface, reflectivity=reflectivity, index=1.5,
                    transparency=0.5)


def test_shares_for_every_surface_kind(example_scenes):
    scene = Scene(bodies=[Sphere((0, 0, -5), 1.0, _material("Diffuse", 0.18)),
                          Sphere((2, 0, -5), 1.0, _material("Reflecting", 0.58, 0.7)),
                          Sphere((4, 0, -5), 1.0, _material("Refractive", 0.9))])
    want = np.array([np.float32(0.18), (np.float32(1.0) - np.float32(0.7)) * np.float32(0.58), np.float32(0.0)], np.float32)
    assert np.array_equal(bits(ambient.shares(scene)), bits(want))
    assert np.array_equal(bits(ambient_ref.shares(scene)), bits(want))
    for name in ("test1", "test2", "test3"):  # the example scenes hold all three kinds between them
        s = example_scenes[name]
        assert np.array_equal(bits(ambient.shares(s)), bits(ambient_ref.shares(s))), name
    kinds = {b.material.surface for n in ("test1", "test2", "test3") for b in example_scenes[n].bodies}
    assert kinds == {"Diffuse", "Reflecting", "Refractive"}


def test_numpy_compose_is_the_reference_and_colour_zero_is_the_resolve():
    rng = np.random.default_rng(5)
    h, w = 13, 29
    samples = rng.uniform(-0.2, 1.4, (2 * h, 2 * w, 3)).astype(np.float32)
    samples[0, 0, 0] = np.nan
    mean, resolved = aa.resolve_box(samples, 2)  # the clamped means and rg_render_image_aa's bytes
    albedo = rng.random((h, w, 3), dtype=np.float32)
    body = rng.integers(-1, 4, (h, w)).astype(np.int32)
    aof = rng.random((h, w), dtype=np.float32)
    share = np.array([0.18, 0.3, 0.0, 0.9], np.float32)
    for color in ((0.3, 0.25, 0.45), 0.2, (5.0, 0.0, 0.5)):
        v, rgba = ambient.compose(mean, albedo, body, aof, share, color)
        v_c, rgba_c = ambient_ref.compose(mean, albedo, body, aof, share, color)
        assert np.array_equal(bits(v), bits(v_c)) and np.array_equal(rgba, rgba_c), color
        assert (rgba[..., 3] == 255).all() and v.min() >= 0 and v.max() <= 1
        miss = body < 0
        assert np.array_equal(rgba[miss], resolved[miss])  # a miss keeps the beauty frame
        assert np.array_equal(rgba[body == 2], resolved[body == 2])  # share 0: so does a refractive body
    v0, rgba0 = ambient.compose(mean, albedo, body, aof, share, 0.0)
    assert np.array_equal(rgba0, resolved) and np.array_equal(ambient_ref.compose(mean, albedo, body, aof, share, 0.0)[1], resolved)
    assert (v != v0).any()


# ---------------------------------------------------------------- 2. the conditions on the inputs
@pytest.mark.parametrize("name", ambient_cases.SCENES)
def test_scene_cases_meet_the_conditions(example_scenes, name):
    ambient_cases.assert_condition(example_scenes, name)


@pytest.mark.parametrize("w,h", [s for s in ambient_cases.SIZES if s[0] * s[1] > 1000])
def test_synthetic_guides_meet_the_conditions(w, h):
    ambient_cases.assert_guides(w, h)


def test_frame_reference_adds_up(example_scenes):
    """ambient_ref.frame: counts are the three passes', the status rule, the unfiltered frame composes the raw pass."""
    name, (k, radius, bias) = "test1", ambient_cases.combos("test1")[0]
    scene = ao_cases.scene(example_scenes, name)
    w, h = 33, 21
    f = ambient_ref.frame(name, scene, w, h, (0.3, 0.25, 0.45), 2, (k, radius, bias), 2, 0.9)
    hit = int((f["body"] >= 0).sum())
    assert f["status"] == 0 and f["error_pixel"] == -1 and f["counts"]["primary"] == w * h * (2 * 2 + 2)
    f0 = ambient_ref.frame(name, scene, w, h, 0.0, 2, (k, radius, bias), 0, 0.9)
    assert np.array_equal(f0["rgba"], f0["beauty_rgba"]) and np.array_equal(bits(f0["aof"]), bits(f0["raw"]))
    assert f["counts"]["shadow"] == f0["counts"]["shadow"] >= k * k * hit
    bad = ao_cases.nan_scene()
    fb = ambient_ref.frame("nan scene", bad, 17, 11, 0.3, 1, (2, INF, 1e-13), 2, 0.9)
    a_st, _, _, a_err, _, _ = ao_ref.render(bad, 17, 11, 2)
    assert fb["status"] == a_st == _abi.RG_ERR_NAN_DISTANCE and fb["error_pixel"] == a_err >= 0


# ---------------------------------------------------------------- 3. the header as a program
def _cxx():
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    return cxx


def test_ambient_header(tmp_path):
    exe = tmp_path / "ambient_test"
    subprocess.run([_cxx(), *CXXFLAGS, "-o", str(exe), str(SRC)], check=True, timeout=300)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"


def test_ambient_header_sanitized(tmp_path):
    """The same program as its own executable under AddressSanitizer + UBSan."""
    exe = tmp_path / "ambient_test_san"
    subprocess.run([_cxx(), *CXXFLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), str(SRC)],
                   check=True, timeout=300)
    env = {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok"


def test_reference_is_written_from_the_header_alone():
    code = re.sub(r"/\*.*?\*/", "", ambient_ref.SRC.read_text(), flags=re.S)
    assert "rg_ambient.h" not in code and "csrc" not in code
    assert re.findall(r'#include "([^"]+)"', code) == ["../../include/raingun.h"]


# ---------------------------------------------------------------- 4. the quality statement
@pytest.mark.parametrize("name,radius", QUALITY_CASES)
def test_filtered_frame_is_closer_to_the_truth(example_scenes, name, radius):
    """Truth: the 3W x 3H k = 8 frame box-averaged 3 x 3 (576 rays per pixel); RMS error over the hit pixels whose
    3 x 3 truth block is one body; the filter: radius 2, normal_min 0.9.  Strictly less error at k = 2, 3 and 4."""
    w, h = QUALITY_SIZE
    scene = ao_cases.scene(example_scenes, name)
    st, fine, _, _, _, _ = ao_ref.render(scene, 3 * w, 3 * h, 8, radius)
    assert st == 0
    blocks = aov_ref.render(scene, 3 * w, 3 * h, layers=("body",))[1]["body"].reshape(h, 3, w, 3)
    one = (blocks == blocks[:, :1, :, :1]).all(axis=(1, 3)) & (blocks[:, 0, :, 0] >= 0)
    assert one.sum() > 0.5 * w * h
    truth = fine.reshape(h, 3, w, 3).astype(np.float64).mean(axis=(1, 3))
    guides = aov_ref.render(scene, w, h, layers=("body", "normal"))[1]

    def rms(frame):
        return float(np.sqrt((((frame.astype(np.float64) - truth)[one]) ** 2).mean()))

    for k in (2, 3, 4):
        raw = ao_ref.render(scene, w, h, k, radius)[1]
        filtered = ambient_ref.filter_ao(raw, guides["body"], guides["normal"], ambient_cases.RADIUS, ambient_cases.NORMAL_MIN)
        e_raw, e_filtered = rms(raw), rms(filtered)
        print(f"{name} radius {radius} k {k}: rms raw {e_raw:.4f} filtered {e_filtered:.4f} ratio {e_filtered / e_raw:.3f}")
        assert e_filtered < e_raw, (name, radius, k, e_raw, e_filtered)


# ---------------------------------------------------------------- 5. bindings, rejections, command lines, build
def test_layouts_and_symbols():
    text = (REPO / "include" / "raingun.h").read_text()

    def fields(struct):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S)
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        return [n for _, n in re.findall(r"^\s*(uint32_t|float|rg_ao)\s+(\w+)(?:\[\d+\])?;", body, re.M)]

    assert fields("rg_ao_filter_desc") == [f[0] for f in _abi.rg_ao_filter_desc._fields_] == ["radius", "normal_min"]
    assert fields("rg_ambient") == [f[0] for f in _abi.rg_ambient._fields_]
    assert C.sizeof(_abi.rg_ao_filter_desc) == 8 and C.sizeof(_abi.rg_ambient) == 48
    assert _abi.rg_ambient.ao.offset == 16 and _abi.rg_ambient.filter_radius.offset == 40
    new = ("rg_ao_filter", "rg_ao_filter_async", "rg_render_image_ambient", "rg_render_ambient_async")
    assert set(new) <= set(_abi.EXPORTED_SYMBOLS)
    lib = _abi.lib()
    for sym in new:
        assert getattr(lib, sym) is not None


def test_rejections_without_a_device():
    lib = _abi.lib()
    INVALID = _abi.RG_ERR_INVALID_ARGUMENT
    ao, body, normal = ambient_cases.guides(17, 3)
    out = np.full((3, 17), 7.0, np.float32)
    a, b, n, o = ao.ctypes.data, body.ctypes.data, normal.ctypes.data, out.ctypes.data
    good = _abi.rg_ao_filter_desc(2, 0.9)
    nan = float("nan")
    for f in (_abi.rg_ao_filter_desc(0, 0.9), _abi.rg_ao_filter_desc(9, 0.9), _abi.rg_ao_filter_desc(2, nan),
              _abi.rg_ao_filter_desc(2, -0.5), _abi.rg_ao_filter_desc(2, 1.5)):
        assert lib.rg_ao_filter(0, a, b, n, 17, 3, C.byref(f), o) == INVALID
        assert lib.rg_ao_filter_async(0, a, b, n, 17, 3, C.byref(f), o, None) == INVALID
    for args in ((None, b, n, 17, 3), (a, None, n, 17, 3), (a, b, None, 17, 3), (a, b, n, 0, 3), (a, b, n, 17, 0),
                 (a, b, n, 1 << 16, 1 << 16)):
        assert lib.rg_ao_filter(0, *args, C.byref(good), o) == INVALID
    assert lib.rg_ao_filter(0, a, b, n, 17, 3, None, o) == INVALID
    assert lib.rg_ao_filter(0, a, b, n, 17, 3, C.byref(good), None) == INVALID
    assert lib.rg_ao_filter(0, a, b, n, 17, 3, C.byref(good), a) == INVALID  # ao_out may not alias ao_in
    assert lib.rg_ao_filter(-1, a, b, n, 17, 3, C.byref(good), o) == INVALID
    m = _abi.rg_ambient((C.c_float * 3)(0.1, 0.1, 0.1), 1, _abi.rg_ao(2, 0, INF, 1e-13), 2, 0.9)
    rgba = np.full((3, 17, 4), 7, np.uint8)
    assert lib.rg_render_image_ambient(None, 17, 3, C.byref(m), rgba.ctypes.data, None, o, None) == INVALID
    assert lib.rg_render_ambient_async(None, 17, 3, C.byref(m), rgba.ctypes.data, None, o, None, None) == INVALID
    assert (out == 7.0).all() and (rgba == 7).all()  # a rejected call writes nothing


def test_cli_flags():
    yml = str(REPO / "tests" / "golden" / "examples" / "test1.yml")
    o = parse_arguments([yml])
    assert o.ambient is None and o.ao_filter is None
    o = parse_arguments([yml, "--ao", "2", "--ambient", "0.25"])
    assert o.ambient == (0.25, 0.25, 0.25) and o.ao_filter is None and o.ao == (2, INF, 1e-13)
    o = parse_arguments([yml, "--ao", "3,8", "--ambient", "0.5,0.25,1", "--ao-filter", "3,0.5", "--samples", "2",
                         "--aperture", "0.5", "--focus", "30", "--light-radius", "0.5", "--eye", "1,2,3"])
    assert o.ambient == (0.5, 0.25, 1.0) and o.ao_filter == (3, 0.5) and o.samples == 2 and o.lens is not None
    assert parse_arguments([yml, "--ao", "2", "--ao-filter", "0"]).ao_filter == (0, float(np.float32(0.9)))
    assert ambient.parse_spec("0") == (0.0, 0.0, 0.0) and ambient.parse_filter_spec("8,1") == (8, 1.0)
    assert ambient.DEFAULT_FILTER == (2, 0.9)
    for bad in ("", "x", "0.1,0.2", "0.1,0.2,0.3,0.4", "-0.1", "0.1,-0.2,0.3", "inf", "nan", "1e39", "0.1,,0.2", "0.1, 0.2,0.3", "0x1p-2", "1_0",
                "infinity", "0.5f"):
        with pytest.raises(ValueError):
            ambient.parse_spec(bad)
        with pytest.raises(SystemExit, match="Could not parse ambient"):
            parse_arguments([yml, "--ao", "2", f"--ambient={bad}"])
    for bad in ("", "x", "9", "-1", "2,", "2,1.5", "2,-0.1", "2,nan", "2,0.5,1", "2.5", "2,0x1p-1", "2,0_9", "1_0", "2,inf"):
        with pytest.raises(ValueError):
            ambient.parse_filter_spec(bad)
        with pytest.raises(SystemExit, match="Could not parse ao-filter"):
            parse_arguments([yml, "--ao", "2", f"--ao-filter={bad}"])
    with pytest.raises(SystemExit, match="ambient needs ao"):
        parse_arguments([yml, "--ambient", "0.2"])
    with pytest.raises(SystemExit, match="ao-filter needs ao"):
        parse_arguments([yml, "--ao-filter", "2"])
    with pytest.raises(SystemExit, match="ambient cannot be used with adaptive"):
        parse_arguments([yml, "--ambient", "0.2", "--ao", "2", "--samples", "2", "--adaptive", "10"])


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_ambient_units_compile_and_are_in_the_build():
    csrc = REPO / "raingun_amd" / "csrc"
    make = (csrc / "Makefile").read_text()
    assert "rg_ao_filter.hip" in make and "rg_ambient.hip" in make and "rg_ambient.h" in make
    text = (csrc / "rg_ao_filter.hip").read_text()
    assert '#include "rg_ambient.h"' in text and "rg_render_kernel.h" not in text and "rg_k_" not in text
    cmd = [HIPCC, "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fsyntax-only", "-Werror=return-type"]
    procs = [subprocess.Popen(cmd + [f], cwd=csrc, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
             for f in ("rg_ao_filter.hip", "rg_ambient.hip")]
    for p in procs:
        err = p.communicate(timeout=900)[1]
        assert p.returncode == 0 and " error:" not in err, err[-3000:]
