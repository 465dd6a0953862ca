"""The thin lens on the GPU (rg_scene_set_lens; the lens family of rg_render_kernel under rg_render_image_aa and
rg_render_aa_async) against the lens reference of tests/lens_ref.py, which tests/test_lens_cpu.py ties to
the camera reference and the pinned oracle.

The bar is the project's: RGBA8 byte-identical, f32 means within 1e-4, per-class ray counts equal, on both
kernel paths (rg_debug_set_path).  Frames are small (40x30 and 97x61 output pixels, k = 2 and 3: partial
tiles, more than one block, and with 8-row bands several bands and a partial last one); every reference
frame is computed once and shared read-only.
"""
import copy
import ctypes as C
import subprocess

import numpy as np
import pytest

import lens_ref
from gpu_launch import assert_same_pixels, native_cli_path, png, require_device
from raingun_amd import _abi
from raingun_amd.camera import Camera, Lens
from raingun_amd.color import Color
from raingun_amd.scene import AABB, DeviceScene, Material, Scene
from raingun_amd.synth import synthetic_scene

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4  # tests/test_gpu_camera.py's
PATHS = [_abi.PATH_LIGHT, _abi.PATH_HEAVY]
LENS = Lens(0.5, 40.0)       # the scenes lie 30 to 90 away: most of them out of focus
OTHER = Lens(1.5, 70.0)
LOOK = Camera.look_at((3, 2, -10), (0, 0, -30))
INVALID = _abi.RG_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module", autouse=True)
def _device():
    require_device()


_SCENES = {}


def _scene(example_scenes, name):
    """test1 / test2 / synth64, or <name>d<depth> for a copy with that recursion depth."""
    if name not in _SCENES:
        base, _, d = name.partition("d")
        s = synthetic_scene(64, 8, 8) if base == "synth64" else example_scenes[base]
        if d:
            s = copy.copy(s)
            s.max_recursion_depth = int(d)
        _SCENES[name] = s
    return _SCENES[name]


def _ref(example_scenes, name, cam, lens, w, h, k):
    return lens_ref.cached(name, _scene(example_scenes, name), cam, lens, w, h, k)


def _assert_frame(got_rgba, got_mean, got_counts, ref, what):
    st, rgba, mean, counts, err = ref
    assert_same_pixels(got_rgba, rgba, what)
    if got_mean is not None:
        diff = float(np.abs(got_mean.astype(np.float64) - mean.astype(np.float64)).max())
        assert diff <= RGB_TOL, f"{what}: f32 means differ by {diff}"
    if got_counts is not None:
        assert got_counts == counts, (what, got_counts, counts)


def _compare(example_scenes, name, cam, lens, w, h, k, band_rows=0):
    ref = _ref(example_scenes, name, cam, lens, w, h, k)
    assert ref[0] == 0
    for path in PATHS:
        ds = DeviceScene(_scene(example_scenes, name), path=path)
        try:
            ds.set_camera(cam)
            ds.set_lens(lens)
            ds.set_aa_band_rows(band_rows)
            st = _abi.rg_stats()
            rgba, mean = ds.render_image_aa(w, h, k, want_rgb=True, stats=st)
            _assert_frame(rgba, mean, st.rays.as_dict(), ref, f"{name} {w}x{h} k {k} path {path} bands {band_rows}")
            assert st.error_pixel == -1
            assert np.array_equal(ds.render_image_aa(w, h, k), ref[1])  # without the f32 output
        finally:
            ds.close()


# ---------------------------------------------------------------- 1. frames through the lens
@pytest.mark.parametrize("w,h,k", [(40, 30, 2), (40, 30, 3), (97, 61, 2)])
@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_lens_frames(example_scenes, name, w, h, k):
    _compare(example_scenes, name, None, LENS, w, h, k)


@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_lens_under_a_camera(example_scenes, name):
    _compare(example_scenes, name, LOOK, Lens(0.4, 25.0), 40, 30, 2)


@pytest.mark.parametrize("depth", [0, 5])
@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_lens_depths(example_scenes, name, depth):
    _compare(example_scenes, f"{name}d{depth}", None, LENS, 40, 30, 2)


@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_lens_bands(example_scenes, name):
    """8 output rows per band: 97x61 in eight bands, the last one 5 rows; 40x30 at k = 3 in four, the last 6."""
    _compare(example_scenes, name, None, LENS, 97, 61, 2, band_rows=8)
    _compare(example_scenes, name, None, LENS, 40, 30, 3, band_rows=8)


# ---------------------------------------------------------------- 2. lenses in flight
@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_two_lenses_in_flight(example_scenes, name):
    """Two streams, two lenses set between two rg_render_aa_async calls, no synchronisation in between: the
    lens travels by value in each launch's kernel arguments, and the reset reaches no launch in flight."""
    import torch

    w, h, k = 97, 61, 2
    lenses = [LENS, OTHER]
    refs = [_ref(example_scenes, name, None, l, w, h, k) for l in lenses]
    assert not np.array_equal(refs[0][1], refs[1][1])
    ds = DeviceScene(_scene(example_scenes, name))
    lib = _abi.lib()
    streams = [torch.cuda.Stream() for _ in lenses]
    rgba = [torch.full((h, w, 4), 9, dtype=torch.uint8, device="cuda") for _ in lenses]
    mean = [torch.full((h, w, 3), 9, dtype=torch.float32, device="cuda") for _ in lenses]
    torch.cuda.synchronize()
    try:
        ds.set_aa_band_rows(16)
        for l, s, b, m in zip(lenses, streams, rgba, mean):
            ds.set_lens(l)
            _abi.check(lib.rg_render_aa_async(ds.handle, w, h, k, C.c_void_p(b.data_ptr()), C.c_void_p(m.data_ptr()),
                                              C.c_void_p(s.cuda_stream), None), "rg_render_aa_async")
        ds.set_lens(None)
        torch.cuda.synchronize()
        for i in range(2):
            _assert_frame(rgba[i].cpu().numpy(), mean[i].cpu().numpy(), None, refs[i], f"{name} stream {i}")
        # with stats: synchronous, the reference's counts
        ds.set_lens(OTHER)
        st = _abi.rg_stats()
        _abi.check(lib.rg_render_aa_async(ds.handle, w, h, k, C.c_void_p(rgba[0].data_ptr()), None,
                                          C.c_void_p(streams[0].cuda_stream), C.byref(st)), "rg_render_aa_async")
        _assert_frame(rgba[0].cpu().numpy(), None, st.rays.as_dict(), refs[1], f"{name} with stats")
        assert st.error_pixel == -1
    finally:
        ds.close()


# ---------------------------------------------------------------- 3. what the lens leaves alone
@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_one_ray_entries_ignore_the_lens(example_scenes, name):
    w, h = 97, 61
    for path in PATHS:
        ds = DeviceScene(_scene(example_scenes, name), path=path)
        try:
            def frames():
                st = _abi.rg_stats()
                image = ds.render_image(w, h, stats=st)
                tiles = ds.render_tiles(w, h, 8, 3, 1, want_rgb=True)
                layers = ds.render_aov(w, h)
                one = ds.render_image_aa(w, h, 1, want_rgb=True)
                return image, st.rays.as_dict(), tiles, layers, one

            image0, counts0, tiles0, layers0, one0 = frames()
            ds.set_lens(LENS)
            image1, counts1, tiles1, layers1, one1 = frames()
            assert np.array_equal(image1, image0) and counts1 == counts0, (name, path)
            assert np.array_equal(tiles1[0], tiles0[0]) and np.array_equal(tiles1[1].view(np.uint32), tiles0[1].view(np.uint32))
            for layer in layers0:
                assert np.array_equal(layers1[layer].view(np.uint8), layers0[layer].view(np.uint8)), (name, path, layer)
            # samples == 1: the bytes of rg_render_image, with and without the f32 output
            assert np.array_equal(one1[0], image0) and np.array_equal(one1[1].view(np.uint32), one0[1].view(np.uint32))
            assert np.array_equal(ds.render_image_aa(w, h, 1), image0)
        finally:
            ds.close()


@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_no_lens_is_the_pinhole(example_scenes, name):
    w, h, k = 97, 61, 2
    for path in PATHS:
        ds = DeviceScene(_scene(example_scenes, name), path=path)
        try:
            st0 = _abi.rg_stats()
            rgba0, mean0 = ds.render_image_aa(w, h, k, want_rgb=True, stats=st0)
            ds.set_lens(LENS)
            assert not np.array_equal(ds.render_image_aa(w, h, k), rgba0)  # the lens is seen ...
            for lens in (None, Lens(0.0, 40.0)):  # ... and gone again
                ds.set_lens(LENS)
                ds.set_lens(lens)
                st = _abi.rg_stats()
                rgba, mean = ds.render_image_aa(w, h, k, want_rgb=True, stats=st)
                assert np.array_equal(rgba, rgba0) and np.array_equal(mean.view(np.uint32), mean0.view(np.uint32)), (name, path, lens)
                assert st.rays.as_dict() == st0.rays.as_dict()
        finally:
            ds.close()


# ---------------------------------------------------------------- 4. rejections
def test_rejections(example_scenes):
    lib = _abi.lib()
    w, h, k = 40, 30, 2
    ref = _ref(example_scenes, "test1", None, LENS, w, h, k)
    ds = DeviceScene(_scene(example_scenes, "test1"))
    try:
        ds.set_lens(LENS)
        for aperture, focus in ((-1.0, 40.0), (0.5, 0.0), (0.5, -3.0), (float("nan"), 40.0), (0.5, float("inf")),
                                (float("inf"), 40.0), (0.5, float("nan"))):
            bad = _abi.rg_lens(aperture, focus)
            assert lib.rg_scene_set_lens(ds.handle, C.byref(bad)) == INVALID, (aperture, focus)
        assert lib.rg_scene_set_lens(None, None) == INVALID
        # the adaptive entries, while a lens with aperture > 0 is set
        out = np.zeros((h, w, 4), np.uint8)
        for t in (0, 32):
            assert lib.rg_render_image_aa_adaptive(ds.handle, w, h, k, t, out.ctypes.data, None, None, None) == INVALID
            assert lib.rg_render_aa_adaptive(ds.handle, w, h, k, t, out.ctypes.data, None, None, None, None) == INVALID
        # the scene kept its lens through all of that
        _assert_frame(ds.render_image_aa(w, h, k), None, None, ref, "the scene keeps its lens after a rejected one")
        # a camera without a right axis spans no lens disk: refused for samples >= 2, fine without the lens
        ds.set_camera(Camera(right=(0.0, 0.0, 0.0)))
        assert lib.rg_render_image_aa(ds.handle, w, h, k, out.ctypes.data, None, None) == INVALID
        assert lib.rg_render_image_aa(ds.handle, w, h, 1, out.ctypes.data, None, None) == _abi.RG_OK
        ds.set_camera(None)
        _assert_frame(ds.render_image_aa(w, h, k), None, None, ref, "after the refused camera")
        ds.set_lens(Lens(0.0, 1.0))  # a pinhole: the adaptive entries are back
        assert ds.render_image_aa_adaptive(w, h, k, 32).shape == (h, w, 4)
    finally:
        ds.close()


@pytest.mark.parametrize("path", PATHS)
def test_aabb_normal_error_through_a_lens(path):
    """The reference's AABB-normal assert (bodies.rs:324) through a lens: the lens reference's code, the output
    pixel of its first failing sample (the AA contract), and the frame is still delivered."""
    bad = Scene(bodies=[AABB(((-3e8, -3e8, -7e8), (3e8, 3e8, -5e8)), Material(Color.from_str("#ffffff"), 0.5))])
    lens = Lens(2e7, 6e8)
    w, h, k = 64, 48, 2
    r_st, r_rgba, _, r_counts, r_err = lens_ref.render(bad, None, lens, w, h, k)
    assert r_st == _abi.RG_ERR_AABB_NORMAL and r_err >= 0
    ds = DeviceScene(bad, path=path)
    try:
        ds.set_lens(lens)
        for band_rows in (0, 8):
            ds.set_aa_band_rows(band_rows)
            st = _abi.rg_stats()
            out = np.zeros((h, w, 4), np.uint8)
            status = _abi.lib().rg_render_image_aa(ds.handle, w, h, k, out.ctypes.data, None, C.byref(st))
            assert status == r_st and st.error_pixel == r_err, (band_rows, status, st.error_pixel, r_err)
            assert st.rays.as_dict() == r_counts and np.array_equal(out, r_rgba)
    finally:
        ds.close()


# ---------------------------------------------------------------- 5. the raingun binary, and cli.py
def test_native_cli_lens_flags(example_scenes, golden_dir, tmp_path):
    cli, yml = native_cli_path(), str(golden_dir / "examples" / "test2.yml")
    w, h, k = 40, 30, 2
    out = tmp_path / "lens.png"
    ref = _ref(example_scenes, "test2", None, Lens(0.5, 30.0), w, h, k)
    r = subprocess.run([cli, "-w", str(w), "-h", str(h), "--samples", str(k), "--aperture", "0.5", "--focus=30", "-o", str(out), yml],
                       cwd=golden_dir, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(png(out), ref[1])
    ref = _ref(example_scenes, "test2", LOOK, Lens(0.25, 20.0), w, h, k)
    r = subprocess.run([cli, "-w", str(w), "-h", str(h), "--samples", str(k), "--eye", "3,2,-10", "--look-at", "0,0,-30",
                        "--aperture", "0.25", "--focus", "20", "-o", str(out), yml],
                       cwd=golden_dir, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(png(out), ref[1])
    bad_width = subprocess.run([cli, "--samples", "9", yml], capture_output=True, text=True, timeout=60)
    for flags in (["--aperture", "0.5"], ["--samples", "2", "--focus", "3"], ["--aperture", "0.5", "--focus", "3"],
                  ["--samples", "1", "--aperture", "0.5", "--focus", "3"],
                  ["--samples", "2", "--adaptive", "32", "--aperture", "0.5", "--focus", "3"],
                  ["--samples", "2", "--aperture", "-1", "--focus", "3"], ["--samples", "2", "--aperture", "1", "--focus", "0"],
                  ["--samples", "2", "--aperture", "x", "--focus", "3"], ["--samples", "2", "--aperture", "1", "--focus", "nan"],
                  ["--samples", "2", "--focus", "3", "--aperture"]):
        r = subprocess.run([cli, *flags, "-o", str(tmp_path / "no.png"), yml], capture_output=True, text=True, timeout=60)
        assert r.returncode == bad_width.returncode == 1 and r.stderr.startswith("error:"), (flags, r.returncode, r.stderr)
    assert not (tmp_path / "no.png").exists()


def test_python_cli_lens_flags(example_scenes, golden_dir, tmp_path):
    from raingun_amd.cli import main

    w, h, k = 40, 30, 3
    ref = _ref(example_scenes, "test2", LOOK, Lens(0.25, 20.0), w, h, k)
    out = tmp_path / "lens.png"
    assert main([str(golden_dir / "examples" / "test2.yml"), "-w", str(w), "-h", str(h), "--samples", str(k), "--eye", "3,2,-10",
                 "--look-at", "0,0,-30", "--aperture", "0.25", "--focus", "20", "-o", str(out)]) == 0
    assert np.array_equal(png(out), ref[1])
    scene = copy.copy(_scene(example_scenes, "test2"))
    scene.set_lens(Lens(0.25, 20.0))  # Scene.set_lens: every DeviceScene of the scene starts with it
    assert np.array_equal(scene.render_image(w, h, samples=k, camera=LOOK), ref[1])
    assert scene.lens == Lens(0.25, 20.0) and _scene(example_scenes, "test2").lens is None
