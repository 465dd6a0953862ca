"""The movable camera on the GPU (rg_scene_set_camera; the camera family of rg_render_kernel) against the
camera reference of tests/camera_ref.py, which tests/test_camera_cpu.py ties to the pinned oracle.

The bar is the project's: RGBA8 byte-identical, f32 RGB within 1e-4, per-class ray counts equal, on
both kernel paths (rg_debug_set_path).  Frames are small (97x61, 64x48: odd sizes, partial tiles,
more than one block); every reference frame is computed once and shared read-only.
"""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import camera_ref
from gpu_launch import assert_same_pixels, device_launch, native_cli_path, png, require_device
from raingun_amd import _abi, aa
from raingun_amd.camera import Camera
from raingun_amd.color import Color
from raingun_amd.scene import (AABB, DeviceScene, DirectionalLight, Material, Plane, Scene, SceneDesc, Sphere,
                               SphericalLight)
from raingun_amd.synth import synthetic_scene

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4
PATHS = [_abi.PATH_LIGHT, _abi.PATH_HEAVY]
WHITE = Color.from_str("#ffffff")


@pytest.fixture(scope="module", autouse=True)
def _device():
    require_device()


# ---------------------------------------------------------------- scenes and poses
_SCENES = {}


def _slab_scene():
    """The scene of tests/test_gpu_host_paths.py test_rays_in_aabb_slab_planes: box faces at x = 0, a floor at y = -2."""
    m = Material(WHITE, 0.5)
    return Scene(bodies=[AABB(((0.0, -1.0, -5.0), (1.0, 1.0, -3.0)), m),
                         AABB(((-2.0, -1.5, -4.0), (0.0, -1.0, -2.5)), Material(Color.from_str("#ff8040"), 0.4)),
                         Plane((0.0, -2.0, 0.0), (0.0, -1.0, 0.0), m)],
                 lights=[DirectionalLight((0.0, -1.0, 0.0), WHITE, 1.0), SphericalLight((0.0, 3.0, -4.0), WHITE, 300.0)])


def _scene(example_scenes, name):
    if name not in _SCENES:
        if name.startswith("synth"):  # synth<spheres>[d<depth>]: 8 planes for 64 spheres, 2 otherwise
            n, _, d = name[5:].partition("d")
            s = synthetic_scene(int(n), 8 if int(n) == 64 else 2, 8 if int(n) == 64 else 5)
            if d:
                s.max_recursion_depth = int(d)
        elif name == "slab":
            s = _slab_scene()
        else:
            s = example_scenes[name]
        _SCENES[name] = s
    return _SCENES[name]


def _scaled(cam, forward_scale):
    return Camera(cam.eye, cam.right, cam.up, tuple(c * forward_scale for c in cam.forward))


def _far():
    """An eye 10^4 scene extents (~100) from the scene, which takes the far-origin BVH paths; the
    forward vector is scaled so that the scene still fills the frame (a long lens)."""
    target, away = (0.0, 5.0, -50.0), (0.3, 0.4, 1.0)
    n = 1e6 / (away[0] ** 2 + away[1] ** 2 + away[2] ** 2) ** 0.5
    eye = tuple(t + a * n for t, a in zip(target, away))
    return _scaled(Camera.look_at(eye, target), 1.5e4)


def _inside_glass(scene):
    s = next(b for b in scene.bodies if isinstance(b, Sphere) and b.material.surface == "Refractive")
    eye = (s.center[0] + 0.3 * s.radius, s.center[1] - 0.2 * s.radius, s.center[2] + 0.1 * s.radius)
    return Camera.look_at(eye, (0.0, 4.0, -45.0))


POSES = {
    "look": Camera.look_at((3, 2, -10), (0, 0, -30)),
    "down": Camera.look_at((0.0, 30.0, -40.0), (0.0, 0.0, -40.0), up=(0, 0, -1)),  # straight down
    "far": _far(),
    "sheared": Camera(eye=(1.0, 3.0, 5.0), right=(1.3, 0.2, 0.0), up=(0.3, 0.8, -0.1), forward=(0.1, -0.2, -2.5)),
    # in the floor plane y = -2 and in the box face plane x = 0 (odd widths: a column of rays with d.x == 0)
    "in_planes": Camera.at((0.0, -2.0, 0.0)),
    "in_face": Camera.look_at((0.0, 0.5, 1.0), (0.0, 0.0, -4.0)),
}


def _pose(example_scenes, scene_name, pose):
    if pose == "glass":
        return _inside_glass(_scene(example_scenes, scene_name))
    return POSES[pose]


def _ref(example_scenes, name, cam, w, h, **tiling):
    return camera_ref.cached(name, _scene(example_scenes, name), cam, w, h, **tiling)


def _assert_frame(got_rgba, got_rgb, got_counts, ref, what):
    st, rgba, rgb, counts, err = ref
    assert_same_pixels(got_rgba, rgba, what)
    if got_rgb is not None:
        diff = float(np.abs(got_rgb.astype(np.float64) - rgb.astype(np.float64)).max())
        assert diff <= RGB_TOL, f"{what}: f32 RGB differs by {diff}"
    if got_counts is not None:
        assert got_counts == counts, (what, got_counts, counts)


def _compare(example_scenes, name, cam, w, h, bvh=None):
    ref = _ref(example_scenes, name, cam, w, h)
    assert ref[0] == 0
    for path in PATHS:
        ds = DeviceScene(_scene(example_scenes, name), path=path, bvh=bvh)
        try:
            ds.set_camera(cam)
            st = _abi.rg_stats()
            rgba, rgb = ds.render_tiles(w, h, want_rgb=True, stats=st)
            _assert_frame(rgba, rgb, st.rays.as_dict(), ref, f"{name} {w}x{h} path {path} bvh {bvh}")
            assert st.error_pixel == -1
        finally:
            ds.close()


# ---------------------------------------------------------------- 4. the identity camera, set explicitly
@pytest.mark.parametrize("name,w,h", [("test1", 200, 150), ("test2", 200, 150), ("test3", 200, 150), ("synth64", 97, 61)])
def test_identity_camera_is_no_camera(oracle_lib, example_scenes, name, w, h):
    scene = _scene(example_scenes, name)
    o_st, o_rgba, o_rgb, o_counts, _ = oracle_lib.render(SceneDesc(scene), w, h, want_rgb=True)
    assert o_st == 0
    for path in PATHS:
        ds = DeviceScene(scene, path=path)
        try:
            st0, st1 = _abi.rg_stats(), _abi.rg_stats()
            plain_initial = device_launch(ds, w, h).plain
            rgba0, rgb0 = ds.render_tiles(w, h, want_rgb=True, stats=st0)
            ds.set_camera(Camera.identity())
            rgba1, rgb1 = ds.render_tiles(w, h, want_rgb=True, stats=st1)
            assert np.array_equal(rgba1, rgba0) and np.array_equal(rgba1, o_rgba), (name, path)
            assert float(np.abs(rgb1.astype(np.float64) - o_rgb.astype(np.float64)).max()) <= RGB_TOL
            assert st1.rays.as_dict() == st0.rays.as_dict() == o_counts, (name, path)
            # device-resident launches: PLAIN without a camera (light scenes that qualify), never with
            # one, and again after the reset -- the scene launches what it launched before
            base, counts, plain_before, _ = device_launch(ds, w, h)
            assert plain_before is False
            ds.set_camera(None)
            again, counts_again, plain_after, _ = device_launch(ds, w, h)
            assert np.array_equal(base, o_rgba) and np.array_equal(again, o_rgba)
            assert counts == counts_again == o_counts
            assert plain_after == plain_initial, "set_camera(None) did not bring the scene's own kernel back"
            if name == "test1" and path == _abi.PATH_LIGHT:
                # a frame size whose PLAIN launch tests/test_gpu_light_plain.py pins
                ds.set_camera(Camera.identity())
                assert device_launch(ds, 97, 61).plain is False
                ds.set_camera(None)
                assert device_launch(ds, 97, 61).plain is True, "set_camera(None) did not bring the PLAIN kernel back"
        finally:
            ds.close()


# ---------------------------------------------------------------- 5. the 180-degree fact on the GPU
@pytest.mark.parametrize("w,h", [(64, 48), (97, 61)])
@pytest.mark.parametrize("name", ["synth16", "synth64", "test2"])
def test_turned_camera_on_the_mirrored_scene(oracle_lib, example_scenes, name, w, h):
    scene = _scene(example_scenes, name)
    o_st, o_rgba, o_rgb, o_counts, _ = oracle_lib.render(SceneDesc(scene), w, h, want_rgb=True)
    assert o_st == 0
    mirrored = camera_ref.mirrored_xz(scene)
    for path in PATHS:
        for bvh in ((True, False) if name != "test2" else (None,)):
            ds = DeviceScene(mirrored, path=path, bvh=bvh)
            try:
                ds.set_camera(camera_ref.TURNED)
                st = _abi.rg_stats()
                rgba, rgb = ds.render_tiles(w, h, want_rgb=True, stats=st)
                _assert_frame(rgba, rgb, st.rays.as_dict(), (0, o_rgba, o_rgb, o_counts, -1), f"{name} path {path} bvh {bvh}")
            finally:
                ds.close()


# ---------------------------------------------------------------- 6. general poses
@pytest.mark.parametrize("name,pose,w,h", [
    ("test1", "look", 97, 61), ("test1", "down", 64, 48), ("test1", "sheared", 97, 61), ("test1", "far", 64, 48),
    ("test3", "look", 64, 48), ("test3", "down", 97, 61), ("test3", "sheared", 64, 48), ("test3", "far", 97, 61),
    ("synth64", "look", 97, 61), ("synth64", "down", 64, 48), ("synth64", "far", 97, 61), ("synth64", "glass", 64, 48),
    ("synth64", "sheared", 64, 48), ("synth1024", "look", 64, 48), ("synth1024", "far", 64, 48),
    ("synth1024", "glass", 64, 48), ("slab", "in_planes", 33, 21), ("slab", "in_planes", 65, 37),
    ("slab", "in_face", 33, 21), ("slab", "in_face", 65, 37),
])
def test_general_poses(example_scenes, name, pose, w, h):
    _compare(example_scenes, name, _pose(example_scenes, name, pose), w, h)


@pytest.mark.parametrize("bvh", [True, False])
def test_far_eye_with_and_without_bvh(example_scenes, bvh):
    _compare(example_scenes, "synth64", POSES["far"], 97, 61, bvh=bvh)
    _compare(example_scenes, "synth64", POSES["look"], 97, 61, bvh=bvh)


@pytest.mark.parametrize("depth", [0, 1, 5, 66])
def test_depths(example_scenes, depth):
    _compare(example_scenes, f"synth64d{depth}", POSES["look"], 64, 48)
    s = copy.copy(example_scenes["test1"])
    s.max_recursion_depth = depth
    _SCENES.setdefault(f"test1d{depth}", s)
    _compare(example_scenes, f"test1d{depth}", POSES["look"], 97, 61)


# ---------------------------------------------------------------- 7. every entry point, one camera
ENTRY_SCENES = ["test1", "synth64"]  # a light-path and a heavy-path scene


@pytest.mark.parametrize("name", ENTRY_SCENES)
def test_render_tiles_tilings(example_scenes, name):
    w, h, cam = 97, 61, POSES["look"]
    ds = DeviceScene(_scene(example_scenes, name))
    try:
        ds.set_camera(cam)
        for rows, stride, offset in ((8, 3, 1), (16, 2, 0)):
            ref = _ref(example_scenes, name, cam, w, h, tile_rows=rows, stride=stride, offset=offset)
            st = _abi.rg_stats()
            rgba, rgb = ds.render_tiles(w, h, rows, stride, offset, want_rgb=True, stats=st)
            _assert_frame(rgba, rgb, st.rays.as_dict(), ref, f"{name} tiling {rows, stride, offset}")
        ref = _ref(example_scenes, name, cam, w, h)
        st = _abi.rg_stats()
        _assert_frame(ds.render_image(w, h, stats=st), None, st.rays.as_dict(), ref, f"{name} render_image")
    finally:
        ds.close()


@pytest.mark.parametrize("name", ENTRY_SCENES)
def test_render_stream_and_cancel(example_scenes, name):
    w, h, cam = 97, 61, POSES["look"]
    ref = _ref(example_scenes, name, cam, w, h)
    ds = DeviceScene(_scene(example_scenes, name))
    try:
        ds.set_camera(cam)
        got = np.zeros_like(ref[1])
        seen = []
        st = _abi.rg_stats()
        _abi.check(ds.render_stream(w, h, lambda r, b: (got.__setitem__(slice(r, r + b.shape[0]), b), seen.append(r))[0], 16, st))
        assert seen == list(range(0, h, 16))
        _assert_frame(got, None, st.rays.as_dict(), ref, f"{name} stream")
        calls = []
        status = ds.render_stream(w, h, lambda r, b: calls.append((r, b)) or len(calls) == 2, 16)
        assert status == _abi.RG_ERR_CANCELLED and [r for r, _ in calls] == [0, 16]
        for r, b in calls:  # the bands delivered before the cancel are the camera's
            assert np.array_equal(b, ref[1][r:r + b.shape[0]])
        _assert_frame(ds.render_image(w, h), None, None, ref, f"{name} after the cancel")
    finally:
        ds.close()


@pytest.mark.parametrize("name", ENTRY_SCENES)
def test_supersampled_frames(example_scenes, name):
    w, h, k, t, cam = 97, 61, 2, 32, POSES["look"]
    base = _ref(example_scenes, name, cam, w, h)
    samples = _ref(example_scenes, name, cam, k * w, k * h)
    want_mean, want_rgba = aa.resolve_box(samples[2], k)
    ad_mean, ad_rgba, ad_mask = aa.resolve_adaptive(base[1], base[2], samples[2], k, t)
    flagged = int(ad_mask.sum())
    assert 0 < flagged < w * h
    for path in PATHS:
        ds = DeviceScene(_scene(example_scenes, name), path=path)
        try:
            ds.set_camera(cam)
            st = _abi.rg_stats()
            rgba, mean = ds.render_image_aa(w, h, k, want_rgb=True, stats=st)
            assert np.array_equal(rgba, want_rgba), (name, path)
            assert float(np.abs(mean.astype(np.float64) - want_mean.astype(np.float64)).max()) <= RGB_TOL
            assert st.rays.as_dict() == samples[3]
            st = _abi.rg_stats()
            rgba, mean, mask = ds.render_image_aa_adaptive(w, h, k, t, want_rgb=True, want_mask=True, stats=st)
            assert np.array_equal(mask, ad_mask), (name, path)
            assert np.array_equal(rgba, ad_rgba), (name, path, int(np.count_nonzero((rgba != ad_rgba).any(axis=2))))
            assert float(np.abs(mean.astype(np.float64) - ad_mean.astype(np.float64)).max()) <= RGB_TOL
            assert st.rays.primary == w * h + k * k * flagged
        finally:
            ds.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ENTRY_SCENES)
def test_render_multi_stand_in(example_scenes, name, mode):
    w, h, cam = 97, 61, POSES["look"]
    ref = _ref(example_scenes, name, cam, w, h)
    other = _ref(example_scenes, name, POSES["down"], w, h)
    ds = DeviceScene(_scene(example_scenes, name))
    try:
        ds.set_multi(mode, stand_in=True, bands=0)
        ds.set_camera(cam)
        st = _abi.rg_stats()
        _assert_frame(ds.render_multi(w, h, 3, 8, stats=st), None, st.rays.as_dict(), ref, f"{name} multi mode {mode}")
        ds.set_camera(POSES["down"])  # the replicas exist now: they follow
        st = _abi.rg_stats()
        _assert_frame(ds.render_multi(w, h, 3, 8, stats=st), None, st.rays.as_dict(), other, f"{name} multi, next camera")
    finally:
        ds.close()


GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p)


@pytest.mark.parametrize("name", ENTRY_SCENES)
def test_frames_loop_world_1(example_scenes, name):
    """rg_frames_* with one rank (a stand-in gather that copies the rank's own part, as ncclGather would)."""
    import torch

    hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    fn = GATHER_FN(lambda send, recv, count, dtype, root, comm, stream: hip.hipMemcpyAsync(recv, send, count, 3, stream))
    w, h, depth = 97, 61, 3
    cams = [POSES["look"], POSES["down"]]
    refs = [_ref(example_scenes, name, c, w, h) for c in cams]
    ds = DeviceScene(_scene(example_scenes, name))
    lib = _abi.lib()
    hdl = C.c_void_p()
    _abi.check(lib.rg_frames_create(ds.handle, w, h, 8, 0, 1, depth, C.c_void_p(1), C.cast(fn, C.c_void_p), C.byref(hdl)))
    try:
        out = np.empty((h, w, 4), np.uint8)
        for k in range(2 * depth + 1):  # a camera per frame: frame k is seen through cams[k % 2]
            ds.set_camera(cams[k % 2])
            _abi.check(lib.rg_frames_step(hdl))
            if k % 2 == 0 or k == 2 * depth:
                _abi.check(lib.rg_frames_flush(hdl))
                _abi.check(lib.rg_frames_read_image(hdl, out.ctypes.data))
                _assert_frame(out, None, None, refs[k % 2], f"{name} frame {k}")
    finally:
        lib.rg_frames_destroy(hdl)
        ds.close()


# ---------------------------------------------------------------- 8. cameras in flight
@pytest.mark.parametrize("name", ENTRY_SCENES)
def test_three_cameras_in_flight(example_scenes, name):
    """Three streams, three cameras set between three rg_render_tiles_async launches, no synchronisation
    in between: the camera travels by value in each launch's kernel arguments."""
    import torch

    w, h = 97, 61
    cams = [POSES["look"], POSES["down"], POSES["sheared"]]
    refs = [_ref(example_scenes, name, c, w, h) for c in cams]
    ds = DeviceScene(_scene(example_scenes, name))
    lib = _abi.lib()
    streams = [torch.cuda.Stream() for _ in cams]
    bufs = [torch.full((h, w, 4), 9, dtype=torch.uint8, device="cuda") for _ in cams]
    t = _abi.rg_tiling(h, 1, 0)
    try:
        for rounds in range(2):  # the second round finds every stream's launch context in place
            for cam, s, b in zip(cams, streams, bufs):
                ds.set_camera(cam)
                _abi.check(lib.rg_render_tiles_async(ds.handle, w, h, C.byref(t), C.c_void_p(b.data_ptr()), None,
                                                     C.c_void_p(s.cuda_stream), None))
            ds.set_camera(None)  # ... nor does the reset reach a launch in flight
            torch.cuda.synchronize()
            for k, (b, s) in enumerate(zip(bufs, streams)):
                _assert_frame(b.cpu().numpy(), None, None, refs[k], f"{name} stream {k} round {rounds}")
                assert ds.stream_status(s.cuda_stream) == (_abi.RG_OK, -1)
                b.fill_(9)
    finally:
        for s in streams:
            ds.release_stream(s.cuda_stream)
        ds.close()


# ---------------------------------------------------------------- 9. errors
@pytest.mark.parametrize("path", PATHS)
def test_aabb_normal_error_under_a_camera(path):
    """The reference's AABB-normal assert (bodies.rs:324) seen from elsewhere: the same code and first pixel
    as the camera reference, and the frame is still delivered."""
    bad = Scene(bodies=[AABB(((-3e8, -3e8, -7e8), (3e8, 3e8, -5e8)), Material(WHITE, 0.5))])
    cam = Camera.look_at((1e8, 2e8, 3e8), (0.0, 0.0, -6e8))
    w, h = 64, 48
    r_st, r_rgba, _, r_counts, r_err = camera_ref.render(bad, cam, w, h)
    assert r_st == _abi.RG_ERR_AABB_NORMAL and r_err >= 0
    ds = DeviceScene(bad, path=path)
    try:
        ds.set_camera(cam)
        st = _abi.rg_stats()
        out = np.zeros((h, w, 4), np.uint8)
        status = _abi.lib().rg_render_image(ds.handle, w, h, out.ctypes.data, C.byref(st))
        assert status == r_st and st.error_pixel == r_err
        assert st.rays.as_dict() == r_counts and np.array_equal(out, r_rgba)
    finally:
        ds.close()


def test_abi_rejections(example_scenes):
    lib = _abi.lib()
    D3 = C.c_double * 3
    out = _abi.rg_camera()
    INVALID = _abi.RG_ERR_INVALID_ARGUMENT
    assert lib.rg_camera_look_at(D3(3, 2, -10), D3(0, 0, -30), D3(0, 1, 0), C.byref(out)) == _abi.RG_OK
    want = Camera.look_at((3, 2, -10), (0, 0, -30))
    assert (tuple(out.eye), tuple(out.right), tuple(out.up), tuple(out.forward)) == (want.eye, want.right, want.up, want.forward)
    assert lib.rg_camera_look_at(D3(1, 2, 3), D3(1, 2, 3), D3(0, 1, 0), C.byref(out)) == INVALID  # target == eye
    assert lib.rg_camera_look_at(D3(0, 0, 0), D3(0, 0, -5), D3(0, 0, 3), C.byref(out)) == INVALID  # up along the view
    assert lib.rg_camera_look_at(D3(0, 0, 0), D3(0, float("nan"), -5), D3(0, 1, 0), C.byref(out)) == INVALID
    assert lib.rg_camera_look_at(D3(float("inf"), 0, 0), D3(0, 0, -5), D3(0, 1, 0), C.byref(out)) == INVALID
    assert lib.rg_camera_look_at(D3(0, 0, 0), D3(0, 0, -5), D3(0, 1, 0), None) == INVALID
    assert tuple(out.forward) == want.forward  # a rejected call writes nothing
    w, h = 64, 48
    ds = DeviceScene(example_scenes["test2"])
    try:
        ds.set_camera(POSES["look"])
        ref = _ref(example_scenes, "test2", POSES["look"], w, h)
        for member, value in (("forward", (0.0, -0.0, 0.0)), ("eye", (0.0, float("nan"), 0.0)),
                              ("right", (float("inf"), 0.0, 0.0)), ("up", (0.0, 0.0, float("-inf")))):
            bad = camera_ref.c_camera(Camera.identity())
            setattr(bad, member, D3(*value))
            assert lib.rg_scene_set_camera(ds.handle, C.byref(bad)) == INVALID, member
        assert lib.rg_scene_set_camera(None, None) == INVALID
        _assert_frame(ds.render_image(w, h), None, None, ref, "the scene keeps its camera after a rejected one")
    finally:
        ds.close()


# ---------------------------------------------------------------- 10. the raingun binary, and cli.py
def test_native_cli_camera_flags(example_scenes, golden_dir, tmp_path):
    cli, yml = native_cli_path(), str(golden_dir / "examples" / "test2.yml")
    w, h = 97, 61
    cam = Camera.look_at((3, 2, -10), (0, 0, -30))
    ref = _ref(example_scenes, "test2", cam, w, h)
    out = tmp_path / "cam.png"
    r = subprocess.run([cli, "-w", str(w), "-h", str(h), "--eye", "3,2,-10", "--look-at=0,0,-30", "-o", str(out), yml],
                       cwd=golden_dir, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(png(out), ref[1])
    ref = _ref(example_scenes, "test2", Camera.at((-1.0, 2.0, 3.0)), w, h)
    r = subprocess.run([cli, "-w", str(w), "-h", str(h), "--eye", "-1,2,3", "-o", str(out), yml],
                       cwd=golden_dir, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(png(out), ref[1])
    bad_width = subprocess.run([cli, "--samples", "9", yml], capture_output=True, text=True, timeout=60)
    for flags in (["--eye", "1,2"], ["--eye", "1,2,x"], ["--look-at", "1,2,3", "--eye", "1,2,3"], ["--up", "0,1,0"],
                  ["--look-at", "0,0,-5", "--up", "0,0,1"], ["--eye"]):
        r = subprocess.run([cli, *flags, "-o", str(tmp_path / "no.png"), yml], capture_output=True, text=True, timeout=60)
        assert r.returncode == bad_width.returncode == 1 and r.stderr.startswith("error:"), (flags, r.returncode, r.stderr)
    assert not (tmp_path / "no.png").exists()


def test_python_cli_camera_flags(example_scenes, golden_dir, tmp_path):
    from raingun_amd.cli import main

    w, h = 97, 61
    cam = Camera.look_at((3, 2, -10), (0, 0, -30), (0.1, 1, 0))
    ref = _ref(example_scenes, "test2", cam, w, h)
    out = tmp_path / "cam.png"
    assert main([str(golden_dir / "examples" / "test2.yml"), "-w", str(w), "-h", str(h), "--eye", "3,2,-10",
                 "--look-at", "0,0,-30", "--up", "0.1,1,0", "-o", str(out)]) == 0
    assert np.array_equal(png(out), ref[1])
    scene = _scene(example_scenes, "test2")
    assert np.array_equal(scene.render_image(w, h, camera=cam), ref[1])
