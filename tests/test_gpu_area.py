"""Area lights on the GPU (rg_scene_set_light_radii; the area family of rg_render_kernel under rg_render_image_aa
and rg_render_aa_async) against the area reference of tests/area_ref.py, which tests/test_area_cpu.py ties to
the lens and camera references and through them to the pinned oracle.

The bar is the project's: RGBA8 byte-identical, f32 means within 1e-4, per-class ray counts equal, on both
kernel paths (rg_debug_set_path) where the scene admits both.  Frames are small (40x30 and 97x61 output
pixels, k = 2 and 3: partial tiles, more than one block, and with 8-row bands several bands and a partial last
one); every reference frame is computed once and shared read-only.  Every test here calls
rg_scene_set_light_radii, which the parent of this feature does not have.
"""
import copy
import ctypes as C
import subprocess

import numpy as np
import pytest

import area_ref
from gpu_launch import assert_same_pixels, native_cli_path, png, require_device
from mixed_scenes import config_scene
from raingun_amd import _abi
from raingun_amd.camera import Camera, Lens
from raingun_amd.color import Color
from raingun_amd.scene import AABB, DeviceScene, DirectionalLight, Material, Plane, Scene, Sphere, SphericalLight
from raingun_amd.synth import synthetic_scene

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4  # tests/test_gpu_camera.py's
PATHS = [_abi.PATH_LIGHT, _abi.PATH_HEAVY]
LENS = Lens(0.5, 40.0)
LOOK = Camera.look_at((3, 2, -10), (0, 0, -30))
INVALID = _abi.RG_ERR_INVALID_ARGUMENT
MIXED = ("light1_d16", "bvh17", "heavy32", "heavy5l", "light0")
SIZES = [(40, 30, 2), (40, 30, 3), (97, 61, 2)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    require_device()


_SCENES = {}


def refractive_scene():
    """Five glass spheres and a mirror one over a diffuse floor under two spherical lights: every primary ray
    through a sphere opens two subtrees, which a small heavy launch publishes to its block's task pool."""
    glass = lambda c: Material(Color(*c), 0.5, "Refractive", index=1.5, transparency=0.9)
    bodies = [Sphere((-4.0 + 2.0 * i, 0.25 * i, -8.0 - 1.5 * (i % 3)), 0.9 + 0.1 * i,
                     glass((1.0 - 0.1 * i, 0.8, 0.6 + 0.1 * i))) for i in range(5)]
    bodies.append(Sphere((0.5, 3.0, -12.0), 1.5, Material(Color(0.9, 0.9, 1.0), 0.5, "Reflecting", reflectivity=0.5)))
    bodies.append(Plane((0.0, -2.0, 0.0), (0.0, -1.0, 0.0), Material(Color(0.9, 0.9, 0.9), 0.5)))
    return Scene(default_color=Color(0.125, 0.25, 0.375), max_recursion_depth=6, bodies=bodies,
                 lights=[SphericalLight((3.0, 6.0, -4.0), Color(1.0, 0.95, 0.9), 3000.0),
                         SphericalLight((-5.0, 4.0, -9.0), Color(0.7, 0.8, 1.0), 2000.0)])


def _scene(example_scenes, name):
    """test1 / test2 / synth64 / refractive / a tests/mixed_scenes.py config, or <name>@<depth> for a copy with that
    recursion depth."""
    if name not in _SCENES:
        base, _, d = name.partition("@")
        s = (synthetic_scene(64, 8, 8) if base == "synth64" else refractive_scene() if base == "refractive"
             else example_scenes[base] if base in example_scenes else config_scene(base))
        if d:
            s = copy.copy(s)
            s.max_recursion_depth = int(d)
        _SCENES[name] = s
    return _SCENES[name]


def radii_of(scene, scale=1.0):
    """Mixed radii: 0 for a directional light (every scene here with lights but `refractive` has one) and for
    the third light of a scene with more than three; the others 0.4, 0.7, 1.0, .. by index, times `scale`."""
    return tuple(0.0 if isinstance(l, DirectionalLight) or (len(scene.lights) > 3 and i == 2) else scale * (0.4 + 0.3 * i)
                 for i, l in enumerate(scene.lights))


def _paths(scene):
    return PATHS if len(scene.lights) <= 3 else [_abi.PATH_HEAVY]  # more lights than a light kernel's batch: heavy only


def _ref(example_scenes, name, cam, lens, radii, w, h, k):
    return area_ref.cached(name, _scene(example_scenes, name), cam, lens, radii, w, h, k)


def _assert_frame(got_rgba, got_mean, got_counts, ref, what):
    st, rgba, mean, counts, err = ref
    assert_same_pixels(got_rgba, rgba, what)
    if got_mean is not None:
        diff = float(np.abs(got_mean.astype(np.float64) - mean.astype(np.float64)).max())
        assert diff <= RGB_TOL, f"{what}: f32 means differ by {diff}"
    if got_counts is not None:
        assert got_counts == counts, (what, got_counts, counts)


def _async(ds, w, h, k, stats=True):
    """rg_render_aa_async into device memory -> (rgba, mean, counts or None)."""
    import torch

    rgba = torch.full((h, w, 4), 9, dtype=torch.uint8, device="cuda")
    mean = torch.full((h, w, 3), 9, dtype=torch.float32, device="cuda")
    st = _abi.rg_stats()
    stream = torch.cuda.Stream()
    _abi.check(_abi.lib().rg_render_aa_async(ds.handle, w, h, k, C.c_void_p(rgba.data_ptr()), C.c_void_p(mean.data_ptr()),
                                             C.c_void_p(stream.cuda_stream), C.byref(st) if stats else None),
               "rg_render_aa_async")
    torch.cuda.synchronize()
    assert not stats or st.error_pixel == -1
    return rgba.cpu().numpy(), mean.cpu().numpy(), (st.rays.as_dict() if stats else None)


def _compare(example_scenes, name, cam, lens, w, h, k, band_rows=0, paths=None, radii=None, setup=None, entry="both"):
    scene = _scene(example_scenes, name)
    radii = radii_of(scene) if radii is None else radii
    ref = _ref(example_scenes, name, cam, lens, radii, w, h, k)
    assert ref[0] == 0
    for path in (paths or _paths(scene)):
        ds = DeviceScene(scene, path=path)
        try:
            ds.set_camera(cam)
            ds.set_lens(lens)
            ds.set_light_radii(radii)
            ds.set_aa_band_rows(band_rows)
            if setup:
                setup(ds)
            what = f"{name} {w}x{h} k {k} path {path} bands {band_rows}"
            if entry in ("both", "host"):
                st = _abi.rg_stats()
                rgba, mean = ds.render_image_aa(w, h, k, want_rgb=True, stats=st)
                _assert_frame(rgba, mean, st.rays.as_dict(), ref, what)
                assert st.error_pixel == -1
            if entry in ("both", "async"):
                _assert_frame(*_async(ds, w, h, k), ref, what + " async")
        finally:
            ds.close()
    return ref


# ---------------------------------------------------------------- 1. frames under area lights
@pytest.mark.parametrize("w,h,k", SIZES)
@pytest.mark.parametrize("name", ["test1", "synth64", *MIXED])
def test_area_frames(example_scenes, name, w, h, k):
    _compare(example_scenes, name, None, None, w, h, k)


def test_the_radii_are_seen(example_scenes):
    """No test above passes vacuously: the references with and without radii differ, on both kinds of scene."""
    for name in ("test1", "synth64", "bvh17", "heavy5l"):
        scene = _scene(example_scenes, name)
        a = _ref(example_scenes, name, None, None, radii_of(scene), 40, 30, 2)
        b = _ref(example_scenes, name, None, None, (0.0,) * len(scene.lights), 40, 30, 2)
        assert not np.array_equal(a[1], b[1]), name


# ---------------------------------------------------------------- 2. combinations
@pytest.mark.parametrize("name", ["test1", "synth64", "heavy32"])
def test_area_under_a_camera(example_scenes, name):
    _compare(example_scenes, name, LOOK, None, 40, 30, 2)


@pytest.mark.parametrize("name", ["test1", "synth64", "heavy32"])
def test_area_through_a_lens(example_scenes, name):
    ref = _compare(example_scenes, name, None, LENS, 40, 30, 2)
    scene = _scene(example_scenes, name)
    assert not np.array_equal(ref[1], _ref(example_scenes, name, None, None, radii_of(scene), 40, 30, 2)[1])


@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_area_under_a_camera_through_a_lens(example_scenes, name):
    _compare(example_scenes, name, LOOK, Lens(0.4, 25.0), 40, 30, 3)


@pytest.mark.parametrize("depth", [0, 5])
@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_area_depths(example_scenes, name, depth):
    _compare(example_scenes, f"{name}@{depth}", None, None, 40, 30, 2)


# ---------------------------------------------------------------- 3. bands
@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_area_bands(example_scenes, name):
    """One band, two bands, and 8 output rows per band (97x61 in eight bands, the last one 5 rows): the same
    bytes.  The output pixel's index n counts rows of the whole frame; a band-local row gives another hash."""
    for band_rows in (61, 31, 8):
        _compare(example_scenes, name, None, None, 97, 61, 2, band_rows=band_rows, entry="host")
    _compare(example_scenes, name, None, None, 40, 30, 3, band_rows=8)


# ---------------------------------------------------------------- 4. light buffers, the per-lane walk
@pytest.mark.parametrize("name", ["synth64", "heavy5l"])
def test_area_launches_take_no_light_buffers(example_scenes, name):
    """A BVH scene whose point-light frames use light buffers: under area lights the frame is the reference's
    with rg_debug_set_lightbuf on and off -- a buffer built for the light's centre would lose occluders."""
    scene = _scene(example_scenes, name)
    ds = DeviceScene(scene, path=_abi.PATH_HEAVY)
    try:
        assert ds.lightbuf_count() > 0, "the scene has no light buffers: the test would show nothing"
    finally:
        ds.close()
    big = radii_of(scene, scale=4.0)  # lights as wide as the spheres around them
    for on in (True, False):
        _compare(example_scenes, name, None, None, 97, 61, 2, paths=[_abi.PATH_HEAVY], radii=big,
                 setup=lambda ds: ds.set_lightbuf(on), entry="host")


@pytest.mark.parametrize("lane_depth", [0, 1 << 20])
def test_area_per_lane_walk(example_scenes, lane_depth):
    _compare(example_scenes, "synth64", None, None, 97, 61, 2, paths=[_abi.PATH_HEAVY],
             setup=lambda ds: ds.set_lane_depth(lane_depth), entry="host")


# ---------------------------------------------------------------- 5. task splitting
def test_area_task_splitting(example_scenes):
    """Refractive spheres in ONE small heavy launch (a single band, fewer tiles than RG_HEAVY_TASK_TILES, not
    pipelined): reflection subtrees are traced by other lanes of the block, for their owner's pixel."""
    for w, h, k in ((97, 61, 2), (40, 30, 3)):
        ref = _compare(example_scenes, "refractive", None, None, w, h, k, band_rows=h, paths=[_abi.PATH_HEAVY])
        assert ref[3]["secondary"] > w * h  # more secondary rays than output pixels: plenty of split subtrees


# ---------------------------------------------------------------- 6. two sets of radii in sequence
@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_two_radii_sets_in_sequence(example_scenes, name):
    """Render, set new radii, render: each frame is its own reference's (the call waits for the device, then
    rewrites the table); the first render is asynchronous and is not waited for by the test."""
    import torch

    scene = _scene(example_scenes, name)
    w, h, k = 97, 61, 2
    sets = [radii_of(scene), radii_of(scene, scale=3.0)]
    refs = [_ref(example_scenes, name, None, None, r, w, h, k) for r in sets]
    assert not np.array_equal(refs[0][1], refs[1][1])
    ds = DeviceScene(scene)
    try:
        ds.set_aa_band_rows(16)
        out = []
        stream = torch.cuda.Stream()
        for r in sets:
            rgba = torch.full((h, w, 4), 9, dtype=torch.uint8, device="cuda")
            mean = torch.full((h, w, 3), 9, dtype=torch.float32, device="cuda")
            ds.set_light_radii(r)
            _abi.check(_abi.lib().rg_render_aa_async(ds.handle, w, h, k, C.c_void_p(rgba.data_ptr()), C.c_void_p(mean.data_ptr()),
                                                     C.c_void_p(stream.cuda_stream), None), "rg_render_aa_async")
            out.append((rgba, mean))
        torch.cuda.synchronize()
        for i, (rgba, mean) in enumerate(out):
            _assert_frame(rgba.cpu().numpy(), mean.cpu().numpy(), None, refs[i], f"{name} radii set {i}")
        ds.set_light_radii(sets[0])  # and back
        _assert_frame(ds.render_image_aa(w, h, k), None, None, refs[0], f"{name} the first set again")
    finally:
        ds.close()


# ---------------------------------------------------------------- 7. what the radii leave alone
@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_one_ray_entries_ignore_the_radii(example_scenes, name):
    w, h = 97, 61
    scene = _scene(example_scenes, name)
    for path in PATHS:
        ds = DeviceScene(scene, path=path)
        try:
            def frames():
                st = _abi.rg_stats()
                image = ds.render_image(w, h, stats=st)
                tiles = ds.render_tiles(w, h, 8, 3, 1, want_rgb=True)
                layers = ds.render_aov(w, h)
                one = ds.render_image_aa(w, h, 1, want_rgb=True)
                return image, st.rays.as_dict(), tiles, layers, one

            image0, counts0, tiles0, layers0, one0 = frames()
            ds.set_light_radii(radii_of(scene))
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
def test_zero_radii_are_point_lights(example_scenes, name):
    w, h, k = 97, 61, 2
    scene = _scene(example_scenes, name)
    for path in PATHS:
        ds = DeviceScene(scene, path=path)
        try:
            st0 = _abi.rg_stats()
            rgba0, mean0 = ds.render_image_aa(w, h, k, want_rgb=True, stats=st0)
            ds.set_light_radii(radii_of(scene))
            assert not np.array_equal(ds.render_image_aa(w, h, k), rgba0)  # the radii are seen ...
            for radii in (None, (0.0,) * len(scene.lights)):  # ... and gone again
                ds.set_light_radii(radii_of(scene))
                ds.set_light_radii(radii)
                st = _abi.rg_stats()
                rgba, mean = ds.render_image_aa(w, h, k, want_rgb=True, stats=st)
                assert np.array_equal(rgba, rgba0) and np.array_equal(mean.view(np.uint32), mean0.view(np.uint32)), (name, path, radii)
                assert st.rays.as_dict() == st0.rays.as_dict()
        finally:
            ds.close()


# ---------------------------------------------------------------- 8. rejections
def test_rejections(example_scenes):
    lib = _abi.lib()
    w, h, k = 40, 30, 2
    scene = _scene(example_scenes, "test1")  # directional, spherical, spherical
    radii = radii_of(scene)
    ref = _ref(example_scenes, "test1", None, None, radii, w, h, k)
    ds = DeviceScene(scene)
    try:
        ds.set_light_radii(radii)
        arr = lambda *v: (C.c_double * len(v))(*v)
        assert lib.rg_scene_set_light_radii(None, arr(0.0, 1.0, 1.0), 3) == INVALID
        for n in (0, 2, 4):  # not the scene's light count
            assert lib.rg_scene_set_light_radii(ds.handle, arr(0.0, 1.0, 1.0, 1.0), n) == INVALID, n
        for bad in (-1.0, -1e-300, float("nan"), float("inf"), -float("inf")):
            assert lib.rg_scene_set_light_radii(ds.handle, arr(0.0, 1.0, bad), 3) == INVALID, bad
        assert lib.rg_scene_set_light_radii(ds.handle, arr(0.5, 1.0, 1.0), 3) == INVALID  # a directional light stays hard
        # the adaptive entries, while a radius is > 0
        out = np.zeros((h, w, 4), np.uint8)
        for t in (0, 32):
            assert lib.rg_render_image_aa_adaptive(ds.handle, w, h, k, t, out.ctypes.data, None, None, None) == INVALID
            assert lib.rg_render_aa_adaptive(ds.handle, w, h, k, t, out.ctypes.data, None, None, None, None) == INVALID
        # the scene kept its radii through all of that
        _assert_frame(ds.render_image_aa(w, h, k), None, None, ref, "the scene keeps its radii after rejected ones")
        ds.set_light_radii(None)  # point lights: the adaptive entries are back
        assert ds.render_image_aa_adaptive(w, h, k, 32).shape == (h, w, 4)
        ds.set_light_radii((0.0, 0.0, 0.0))
        assert ds.render_image_aa_adaptive(w, h, k, 32).shape == (h, w, 4)
    finally:
        ds.close()


@pytest.mark.parametrize("path", PATHS)
def test_aabb_normal_error_under_area_lights(path):
    """The reference's AABB-normal assert (bodies.rs:324) of tests/test_gpu_lens.py's scene, here under a light
    with a radius: the area reference's code, the output pixel of its first failing sample (the AA contract),
    and the frame is still delivered."""
    bad = Scene(bodies=[AABB(((-3e8, -3e8, -7e8), (3e8, 3e8, -5e8)), Material(Color.from_str("#ffffff"), 0.5))],
                lights=[SphericalLight((1e8, 2e8, -1e8), Color.from_str("#ffffff"), 1e19)])
    radii = (5e7,)
    w, h, k = 64, 48, 2
    r_st, r_rgba, _, r_counts, r_err = area_ref.render(bad, None, None, radii, w, h, k)
    assert r_st == _abi.RG_ERR_AABB_NORMAL and r_err >= 0
    assert not np.array_equal(r_rgba, area_ref.render(bad, None, None, (0.0,), w, h, k)[1])
    ds = DeviceScene(bad, path=path)
    try:
        ds.set_light_radii(radii)
        for band_rows in (0, 8):
            ds.set_aa_band_rows(band_rows)
            st = _abi.rg_stats()
            out = np.zeros((h, w, 4), np.uint8)
            status = _abi.lib().rg_render_image_aa(ds.handle, w, h, k, out.ctypes.data, None, C.byref(st))
            assert status == r_st and st.error_pixel == r_err, (band_rows, status, st.error_pixel, r_err)
            assert st.rays.as_dict() == r_counts and np.array_equal(out, r_rgba)
    finally:
        ds.close()


# ---------------------------------------------------------------- 9. the raingun binary, and cli.py
def test_native_cli_light_radius(example_scenes, golden_dir, tmp_path):
    cli, yml = native_cli_path(), str(golden_dir / "examples" / "test2.yml")  # directional, spherical
    w, h, k = 40, 30, 2
    out = tmp_path / "area.png"
    ref = _ref(example_scenes, "test2", None, None, (0.0, 0.75), w, h, k)
    assert not np.array_equal(ref[1], _ref(example_scenes, "test2", None, None, (0.0, 0.0), w, h, k)[1])
    r = subprocess.run([cli, "-w", str(w), "-h", str(h), "--samples", str(k), "--light-radius", "0.75", "-o", str(out), yml],
                       cwd=golden_dir, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(png(out), ref[1])
    ref = _ref(example_scenes, "test2", LOOK, Lens(0.25, 20.0), (0.0, 1.25), w, h, k)
    r = subprocess.run([cli, "-w", str(w), "-h", str(h), "--samples", str(k), "--eye", "3,2,-10", "--look-at", "0,0,-30",
                        "--aperture", "0.25", "--focus", "20", "--light-radius=0,1.25", "-o", str(out), yml],
                       cwd=golden_dir, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(png(out), ref[1])
    bad_width = subprocess.run([cli, "--samples", "9", yml], capture_output=True, text=True, timeout=60)
    for flags in (["--light-radius", "0.5"], ["--samples", "1", "--light-radius", "0.5"],
                  ["--samples", "2", "--adaptive", "32", "--light-radius", "0.5"], ["--samples", "2", "--light-radius", "-1"],
                  ["--samples", "2", "--light-radius", "x"], ["--samples", "2", "--light-radius", "1,,2"],
                  ["--samples", "2", "--light-radius", "nan"], ["--samples", "2", "--light-radius", "1,2,3"],
                  ["--samples", "2", "--light-radius"]):
        r = subprocess.run([cli, *flags, "-o", str(tmp_path / "no.png"), yml], cwd=golden_dir, capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == bad_width.returncode == 1 and r.stderr.startswith("error:"), (flags, r.returncode, r.stderr)
    assert not (tmp_path / "no.png").exists()


def test_python_cli_light_radius(example_scenes, golden_dir, tmp_path):
    from raingun_amd.cli import main

    w, h, k = 40, 30, 3
    ref = _ref(example_scenes, "test2", LOOK, None, (0.0, 0.75), w, h, k)
    out = tmp_path / "area.png"
    yml = str(golden_dir / "examples" / "test2.yml")
    assert main([yml, "-w", str(w), "-h", str(h), "--samples", str(k), "--eye", "3,2,-10", "--look-at", "0,0,-30",
                 "--light-radius", "0.75", "-o", str(out)]) == 0
    assert np.array_equal(png(out), ref[1])
    with pytest.raises(SystemExit, match="Could not build the area lights"):  # a list of another length than the lights
        main([yml, "-w", str(w), "-h", str(h), "--samples", str(k), "--light-radius", "1,2,3", "-o", str(tmp_path / "no.png")])
    assert not (tmp_path / "no.png").exists()
    scene = copy.copy(_scene(example_scenes, "test2"))
    scene.set_light_radii((0.0, 0.75))  # Scene.set_light_radii: every DeviceScene of the scene starts with them
    assert np.array_equal(scene.render_image(w, h, samples=k, camera=LOOK), ref[1])
    assert scene.light_radii == (0.0, 0.75) and _scene(example_scenes, "test2").light_radii is None
