"""The ambient occlusion pass on the GPU (rg_render_ao / rg_render_ao_async; csrc/rg_ao.hip) against the
reference of tests/ao_ref.py, which tests/test_ao_cpu.py ties to the pinned oracle twice over.

The bar: `ao` bit-identical to the reference (an integer count over k^2, so nothing else can be right), the ray
counts equal (primary == pixels, shadow == k^2 x hit pixels, secondary == 0) and error_pixel equal.  Frames are
small (1x1, 17x3, 97x61: partial tiles, more than one wave and block; k = 8 at 97x61 is about 380 k rays); every
reference is computed once and shared read-only.  The parity cases and the condition they meet -- enough pixels
strictly between 0 and 1 -- are tests/ao_cases.py's; the condition is asserted here on the reference too.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import ao_cases
import ao_ref
from aov_ref import bits
from ao_cases import H, INF, W
from gpu_launch import native_cli_path, png, require_device
from raingun_amd import _abi, ao
from raingun_amd.camera import Camera
from raingun_amd.color import Color
from raingun_amd.scene import AABB, DeviceScene, Material, Scene
from test_gpu_camera import PATHS, POSES, _scene

pytestmark = pytest.mark.gpu

TILINGS = ((8, 3, 1), (16, 2, 0))
CANARY = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _device():
    require_device()


def _has_bvh(ds):
    return bool(ds.bvh_info().built)


def _assert_frame(got, st, ref, what):
    """got, st: the GPU's frame and stats; ref: ao_ref's tuple."""
    r_st, r_ao, r_counts, r_err, _, _ = ref
    got = np.asarray(got)
    assert got.shape == r_ao.shape and got.dtype == np.float32, (what, got.shape, r_ao.shape)
    same = bits(got) == bits(r_ao)
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} ao values differ"
    assert st.rays.as_dict() == r_counts, (what, st.rays.as_dict(), r_counts)
    assert st.error_pixel == r_err, (what, st.error_pixel, r_err)


def _flavours(ds):
    return (True, False) if _has_bvh(ds) else (None,)


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("name", ao_cases.SCENES)
def test_parity(example_scenes, name):
    """97x61: every path, BVH on and off where one is built, the scene's four (k, radius, bias) cases."""
    ao_cases.assert_condition(example_scenes, name)  # on the reference, not on the GPU's result
    scene = ao_cases.scene(example_scenes, name)
    for path in PATHS:
        ds = DeviceScene(scene, path=path)
        try:
            for bvh in _flavours(ds):
                if bvh is not None:
                    ds.set_bvh(bvh)
                for k, radius, bias in ao_cases.combos(name):
                    ref = ao_cases.ref(example_scenes, name, W, H, k, radius, bias)
                    assert ref[0] == 0 and ref[2]["shadow"] == k * k * int((ref[4] >= 0).sum())
                    st = _abi.rg_stats()
                    got = ds.render_ao(W, H, k, radius, bias, stats=st)
                    _assert_frame(got, st, ref, f"{name} path {path} bvh {bvh} k {k} radius {radius} bias {bias}")
        finally:
            ds.close()


@pytest.mark.parametrize("w,h", ao_cases.SMALL)
@pytest.mark.parametrize("name", ao_cases.SCENES)
def test_small_frames(example_scenes, name, w, h):
    scene = ao_cases.scene(example_scenes, name)
    k, radius, bias = ao_cases.combos(name)[1]
    ref = ao_cases.ref(example_scenes, name, w, h, k, radius, bias)
    for path in PATHS:
        ds = DeviceScene(scene, path=path)
        try:
            st = _abi.rg_stats()
            _assert_frame(ds.render_ao(w, h, k, radius, bias, stats=st), st, ref, f"{name} {w}x{h} path {path}")
        finally:
            ds.close()


# ---------------------------------------------------------------- camera
@pytest.mark.parametrize("name", ["test1", "test3", "synth64"])
def test_identity_camera_is_no_camera(example_scenes, name):
    scene = ao_cases.scene(example_scenes, name)
    k, radius, bias = ao_cases.combos(name)[1]
    for path in PATHS:
        ds = DeviceScene(scene, path=path)
        try:
            st0, st1 = _abi.rg_stats(), _abi.rg_stats()
            base = ds.render_ao(W, H, k, radius, bias, stats=st0)
            ds.set_camera(Camera.identity())
            with_cam = ds.render_ao(W, H, k, radius, bias, stats=st1)
            assert np.array_equal(bits(with_cam), bits(base)), (name, path)
            assert st0.rays.as_dict() == st1.rays.as_dict() and st1.error_pixel == -1
        finally:
            ds.close()


@pytest.mark.parametrize("pose", ["look", "far", "sheared"])
@pytest.mark.parametrize("name", ["test1", "synth64", "slab"])
def test_camera_poses(example_scenes, name, pose):
    cam = POSES[pose]
    scene = ao_cases.scene(example_scenes, name)
    k, radius, bias = ao_cases.combos(name)[2]
    ref = ao_cases.ref(example_scenes, name, W, H, k, radius, bias, cam)
    assert ref[0] == 0
    for path in PATHS:
        ds = DeviceScene(scene, path=path)
        try:
            ds.set_camera(cam)
            for bvh in _flavours(ds):
                if bvh is not None:
                    ds.set_bvh(bvh)
                st = _abi.rg_stats()
                _assert_frame(ds.render_ao(W, H, k, radius, bias, stats=st), st, ref, f"{name} {pose} path {path} bvh {bvh}")
        finally:
            ds.close()


@pytest.mark.parametrize("depth", [0, 1 << 20])
def test_lane_walk_flavours(example_scenes, depth):
    """rg_debug_set_lane_depth(0): rays of every depth walk the BVH per lane, a camera's primary rays too; a large
    depth: no ray does, and the AO rays walk with their wave."""
    name, cam = "synth64", POSES["look"]
    scene = ao_cases.scene(example_scenes, name)
    k, radius, bias = ao_cases.combos(name)[3]
    ds = DeviceScene(scene, path=_abi.PATH_HEAVY)
    try:
        ds.set_lane_depth(depth)
        for c in (None, cam):
            ds.set_camera(c)
            st = _abi.rg_stats()
            ref = ao_cases.ref(example_scenes, name, W, H, k, radius, bias, c)
            _assert_frame(ds.render_ao(W, H, k, radius, bias, stats=st), st, ref, f"lane depth {depth} camera {c is not None}")
    finally:
        ds.close()


# ---------------------------------------------------------------- tilings, streams
@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_tilings(example_scenes, name):
    import torch

    cam = POSES["look"]
    scene = ao_cases.scene(example_scenes, name)
    k, radius, bias = ao_cases.combos(name)[1]
    ds = DeviceScene(scene)
    try:
        for c in (None, cam):
            ds.set_camera(c)
            for rows, stride, offset in TILINGS:
                ref = ao_cases.ref(example_scenes, name, W, H, k, radius, bias, c, tile_rows=rows, stride=stride, offset=offset)
                st = _abi.rg_stats()
                got = ds.render_ao_tiles(W, H, k, radius, bias, rows, stride, offset, stats=st)
                torch.cuda.synchronize()
                got = got.cpu().numpy()
                _assert_frame(got, st, ref, f"{name} tiling {rows, stride, offset} camera {c is not None}")
                if (rows, stride, offset) == (8, 3, 1):  # rows 56..63 of tile 7: 61, 62, 63 are padding
                    assert (bits(got[-3:]) == 0).all()  # +0.0f
    finally:
        ds.close()


@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_three_streams_in_flight(example_scenes, name):
    """Three streams, three cameras and two rg_ao values between three rg_render_ao_async launches, no
    synchronisation in between: each stream has its own launch context, camera and pass travel by value.  A
    beauty frame and an AOV frame on one of the streams afterwards still count their own rays."""
    import torch

    cams = [POSES["look"], POSES["down"], POSES["sheared"]]
    scene = ao_cases.scene(example_scenes, name)
    c1, c2 = ao_cases.combos(name)[1], ao_cases.combos(name)[2]
    passes = [c1, c2, c1]
    refs = [ao_cases.ref(example_scenes, name, W, H, *p, cam) for p, cam in zip(passes, cams)]
    ds = DeviceScene(scene)
    streams = [torch.cuda.Stream() for _ in cams]
    try:
        for rounds in range(2):  # the second round finds every stream's launch context in place
            outs = []
            for cam, p, s in zip(cams, passes, streams):
                ds.set_camera(cam)
                outs.append(ds.render_ao_tiles(W, H, *p, stream=s.cuda_stream))
            ds.set_camera(None)
            torch.cuda.synchronize()
            for i, (out, s) in enumerate(zip(outs, streams)):
                got = out.cpu().numpy()
                assert np.array_equal(bits(got), bits(refs[i][1])), f"{name} stream {i} round {rounds}"
                assert ds.stream_status(s.cuda_stream) == (_abi.RG_OK, -1)
        # a beauty frame on one of the streams afterwards finds its counter set zeroed, an AOV frame after it too
        st = _abi.rg_stats()
        t = _abi.rg_tiling(H, 1, 0)
        rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
        _abi.check(_abi.lib().rg_render_tiles_async(ds.handle, W, H, C.byref(t), C.c_void_p(rgba.data_ptr()), None,
                                                    C.c_void_p(streams[0].cuda_stream), C.byref(st)))
        plain = _abi.rg_stats()
        ds2 = DeviceScene(scene)
        try:
            rgba2 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
            _abi.check(_abi.lib().rg_render_tiles_async(ds2.handle, W, H, C.byref(t), C.c_void_p(rgba2.data_ptr()), None,
                                                        None, C.byref(plain)))
        finally:
            ds2.close()
        assert st.rays.as_dict() == plain.rays.as_dict() and st.rays.primary == W * H and st.error_pixel == -1
        assert bool((rgba == rgba2).all())
        st2 = _abi.rg_stats()
        ds.render_aov_tiles(W, H, stream=streams[0].cuda_stream, stats=st2)
        assert st2.rays.as_dict() == {"primary": W * H, "shadow": 0, "secondary": 0} and st2.error_pixel == -1
        st3 = _abi.rg_stats()
        got = ds.render_ao_tiles(W, H, *c1, stream=streams[0].cuda_stream, stats=st3)
        _assert_frame(got.cpu().numpy(), st3, ao_cases.ref(example_scenes, name, W, H, *c1), f"{name} after the others")
    finally:
        for s in streams:
            ds.release_stream(s.cuda_stream)
        ds.close()


@pytest.mark.parametrize("with_stats", [True, False], ids=["stats", "no_stats"])
def test_tiling_that_selects_no_row(example_scenes, with_stats):
    """16x8 under tiling (8, 2, 1): the frame has tile 0 alone, the tiling takes tiles 1, 3, ..  RG_OK, no ray,
    no store, and nothing enqueued: the counter sets must not flip, or the next launch on the stream would count
    on top of what the frame before left in the other set."""
    import torch

    name, w, h = "test1", 16, 8
    scene = ao_cases.scene(example_scenes, name)
    k, radius, bias = ao_cases.combos(name)[1]
    ref = ao_cases.ref(example_scenes, name, w, h, k, radius, bias)
    ds = DeviceScene(scene)
    stream = torch.cuda.Stream()
    hs = stream.cuda_stream
    try:
        def frame(what):
            st = _abi.rg_stats()
            got = ds.render_ao_tiles(w, h, k, radius, bias, stream=hs, stats=st)
            stream.synchronize()
            _assert_frame(got.cpu().numpy(), st, ref, what)

        frame("the frame before")  # its counts stay in the set the next launch zeroes
        big = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
        v = _abi.rg_ao(k, 0, radius, bias)
        t = _abi.rg_tiling(8, 2, 1)
        assert _abi.lib().rg_tiling_rows(h, C.byref(t)) == 0
        st = _abi.rg_stats()
        st.rays.primary, st.error_pixel = 77, 5
        status = _abi.lib().rg_render_ao_async(ds.handle, w, h, C.byref(t), C.byref(v), C.c_void_p(big.data_ptr() + 2048),
                                               C.c_void_p(hs), C.byref(st) if with_stats else None)
        assert status == _abi.RG_OK
        if with_stats:
            assert st.rays.as_dict() == {"primary": 0, "shadow": 0, "secondary": 0} and st.error_pixel == -1
        frame("the frame after")
        assert bool((big == CANARY).all()), "a store under a tiling that selects nothing"
        assert ds.stream_status(hs) == (_abi.RG_OK, -1)
    finally:
        ds.release_stream(hs)
        ds.close()


# ---------------------------------------------------------------- canary
@pytest.mark.parametrize("tiling", [(H, 1, 0), (8, 3, 1)])
def test_stores_stay_inside_the_output(example_scenes, tiling):
    """The output lies in a canary-filled allocation with guards: no byte outside rows x width x 4 changes."""
    import torch

    name = "test1"
    scene = ao_cases.scene(example_scenes, name)
    k, radius, bias = ao_cases.combos(name)[1]
    rows_t, stride, offset = tiling
    ref = ao_cases.ref(example_scenes, name, W, H, k, radius, bias, tile_rows=rows_t, stride=stride, offset=offset)
    rows = ref[1].shape[0]
    guard, size = 4096, rows * W * 4
    for path in PATHS:
        ds = DeviceScene(scene, path=path)
        try:
            big = torch.full((guard + size + guard,), CANARY, dtype=torch.uint8, device="cuda")
            v = _abi.rg_ao(k, 0, radius, bias)
            t = _abi.rg_tiling(rows_t, stride, offset)
            st = _abi.rg_stats()
            _abi.check(_abi.lib().rg_render_ao_async(ds.handle, W, H, C.byref(t), C.byref(v),
                                                     C.c_void_p(big.data_ptr() + guard), None, C.byref(st)))
            host = big.cpu().numpy()
            got = host[guard:guard + size].view(np.float32).reshape(rows, W)
            _assert_frame(got, st, ref, f"canary path {path} tiling {tiling}")
            assert (host[:guard] == CANARY).all() and (host[guard + size:] == CANARY).all(), f"path {path}: a store outside"
        finally:
            ds.close()


# ---------------------------------------------------------------- errors
@pytest.mark.parametrize("path", PATHS)
def test_aabb_normal_error(path):
    """The reference's AABB-normal assert (bodies.rs:324) on the scene of tests/test_gpu_aov.py: the reference's
    status and first pixel, and the frame is delivered."""
    bad = Scene(bodies=[AABB(((-3e8, -3e8, -7e8), (3e8, 3e8, -5e8)), Material(Color.from_str("#ffffff"), 0.5))])
    w, h, k = 64, 48, 2
    for cam in (None, Camera.look_at((1e8, 2e8, 3e8), (0.0, 0.0, -6e8))):
        ref = ao_ref.render(bad, w, h, k, cam=cam)
        assert ref[0] == _abi.RG_ERR_AABB_NORMAL and ref[3] >= 0
        ds = DeviceScene(bad, path=path)
        try:
            ds.set_camera(cam)
            out = np.full((h, w), 7.0, np.float32)
            v = _abi.rg_ao(k, 0, INF, 1e-13)
            st = _abi.rg_stats()
            assert _abi.lib().rg_render_ao(ds.handle, w, h, C.byref(v), out.ctypes.data, C.byref(st)) == ref[0]
            _assert_frame(out, st, ref, f"aabb normal path {path} camera {cam is not None}")
            with pytest.raises(_abi.RaingunError):
                ds.render_ao(w, h, k)
        finally:
            ds.close()


@pytest.mark.parametrize("path", PATHS)
def test_nan_distance_from_an_occlusion_ray(path):
    """tests/ao_cases.py nan_scene: no primary ray sees a NaN distance, the AO rays do (tests/test_ao_cpu.py
    confirms that on the reference); the reference's status and first pixel, and the frame is delivered."""
    scene, w, h, k = ao_cases.nan_scene(), 17, 11, 2
    ref = ao_ref.render(scene, w, h, k)
    assert ref[0] == _abi.RG_ERR_NAN_DISTANCE and ref[3] >= 0
    ds = DeviceScene(scene, path=path)
    try:
        st = _abi.rg_stats()
        layers = ds.render_aov(w, h, ("body",), stats=st)  # the primary rays alone: RG_OK
        assert st.error_pixel == -1 and (layers["body"] != 0).all()
        out = np.full((h, w), 7.0, np.float32)
        v = _abi.rg_ao(k, 0, INF, 1e-13)
        st = _abi.rg_stats()
        assert _abi.lib().rg_render_ao(ds.handle, w, h, C.byref(v), out.ctypes.data, C.byref(st)) == ref[0]
        _assert_frame(out, st, ref, f"nan distance path {path}")
    finally:
        ds.close()


def test_rejections(example_scenes):
    import torch

    lib = _abi.lib()
    INVALID = _abi.RG_ERR_INVALID_ARGUMENT
    ds = DeviceScene(example_scenes["test2"])
    try:
        buf = np.full(64 * 48, 7.0, np.float32)
        dbuf = torch.full((64 * 48,), 7.0, dtype=torch.float32, device="cuda")
        hp, dp = buf.ctypes.data, C.c_void_p(dbuf.data_ptr())
        good = _abi.rg_ao(2, 0, INF, 1e-13)
        t = _abi.rg_tiling(48, 1, 0)
        nan = float("nan")
        bad_passes = [_abi.rg_ao(0, 0, INF, 0.0), _abi.rg_ao(9, 0, INF, 0.0), _abi.rg_ao(2, 0, 0.0, 0.0),
                      _abi.rg_ao(2, 0, -1.0, 0.0), _abi.rg_ao(2, 0, nan, 0.0), _abi.rg_ao(2, 0, 1.0, -1e-13),
                      _abi.rg_ao(2, 0, 1.0, INF), _abi.rg_ao(2, 0, 1.0, nan)]
        for v in bad_passes:
            assert lib.rg_render_ao(ds.handle, 64, 48, C.byref(v), hp, None) == INVALID
            assert lib.rg_render_ao_async(ds.handle, 64, 48, C.byref(t), C.byref(v), dp, None, None) == INVALID
        assert lib.rg_render_ao(ds.handle, 48, 64, C.byref(good), hp, None) == _abi.RG_ERR_PORTRAIT
        assert lib.rg_render_ao(ds.handle, 64, 48, None, hp, None) == INVALID
        assert lib.rg_render_ao(ds.handle, 64, 48, C.byref(good), None, None) == INVALID
        assert lib.rg_render_ao(ds.handle, 0, 48, C.byref(good), hp, None) == INVALID
        assert lib.rg_render_ao(ds.handle, 1 << 16, 1 << 16, C.byref(good), hp, None) == INVALID
        assert lib.rg_render_ao(None, 64, 48, C.byref(good), hp, None) == INVALID
        assert lib.rg_render_ao_async(ds.handle, 48, 64, C.byref(t), C.byref(good), dp, None, None) == _abi.RG_ERR_PORTRAIT
        assert lib.rg_render_ao_async(ds.handle, 64, 48, C.byref(t), None, dp, None, None) == INVALID
        assert lib.rg_render_ao_async(ds.handle, 64, 48, C.byref(t), C.byref(good), None, None, None) == INVALID
        assert lib.rg_render_ao_async(ds.handle, 64, 48, None, C.byref(good), dp, None, None) == INVALID
        for bad in (_abi.rg_tiling(0, 1, 0), _abi.rg_tiling(8, 0, 0), _abi.rg_tiling(8, 2, 2)):
            assert lib.rg_render_ao_async(ds.handle, 64, 48, C.byref(bad), C.byref(good), dp, None, None) == INVALID
        torch.cuda.synchronize()
        assert (buf == 7.0).all() and bool((dbuf == 7.0).all())  # a rejected call writes nothing
        st = _abi.rg_stats()
        frame = ds.render_ao(64, 48, 2, stats=st)  # and the scene still renders
        assert frame.shape == (48, 64) and st.rays.primary == 64 * 48 and st.rays.shadow % 4 == 0
    finally:
        ds.close()


# ---------------------------------------------------------------- both command lines
CLI_FLAGS = ["--draft", "--eye", "3,2,-10", "--look-at=0,0,-30"]
CLI_CASES = [("2", (2, INF, 1e-13)), ("3,5.0", (3, 5.0, 1e-13))]


def _cli_reference(example_scenes, spec):
    w, h = 800, 600  # --draft
    ref = ao_ref.cached("test1", _scene(example_scenes, "test1"), w, h, *spec, ao_cases.CLI_CAMERA)
    assert ref[0] == 0
    return ao.visualize(ref[1])


def test_native_cli_ao(example_scenes, golden_dir, tmp_path):
    cli, yml = native_cli_path(), str(golden_dir / "examples" / "test1.yml")
    plain = tmp_path / "plain.png"
    r = subprocess.run([cli, *CLI_FLAGS, "-o", str(plain), yml], cwd=golden_dir, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert not list(tmp_path.glob("plain.*.png"))
    for i, (flag, spec) in enumerate(CLI_CASES):
        out = tmp_path / f"cli{i}.png"
        # --samples, --aperture and --light-radius change the beauty frame only: leave them out of the byte comparison
        r = subprocess.run([cli, *CLI_FLAGS, "--ao", flag, "-o", str(out), yml], cwd=golden_dir, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == plain.read_bytes()
        got, want = png(tmp_path / f"cli{i}.ao.png"), _cli_reference(example_scenes, spec)
        assert np.array_equal(got, want), (flag, int((got != want).any(axis=2).sum()))
    bad_width = subprocess.run([cli, "--samples", "9", yml], capture_output=True, text=True, timeout=60)
    for flags in (["--ao", "0"], ["--ao", "9"], ["--ao", "2,"], ["--ao", "2,0"], ["--ao", "2,1,-1"], ["--ao", ""], ["--ao"]):
        r = subprocess.run([cli, *flags, "-o", str(tmp_path / "no.png"), yml], capture_output=True, text=True, timeout=60)
        assert r.returncode == bad_width.returncode == 1 and r.stderr.startswith("error:"), (flags, r.returncode, r.stderr)
    assert not list(tmp_path.glob("no*.png"))
    helptext = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--ao <K[,RADIUS[,BIAS]]>" in helptext


def test_python_cli_ao(example_scenes, golden_dir, tmp_path, monkeypatch):
    from raingun_amd.cli import construct_app, main

    monkeypatch.chdir(golden_dir)  # textures resolve against the working directory
    yml = str(golden_dir / "examples" / "test1.yml")
    plain = tmp_path / "plain.png"
    assert main([yml, *CLI_FLAGS, "-o", str(plain)]) == 0
    for i, (flag, spec) in enumerate(CLI_CASES):
        out = tmp_path / f"py{i}.png"
        assert main([yml, *CLI_FLAGS, "--ao", flag, "-o", str(out)]) == 0
        assert out.read_bytes() == plain.read_bytes()
        got, want = png(tmp_path / f"py{i}.ao.png"), _cli_reference(example_scenes, spec)
        assert np.array_equal(got, want), (flag, int((got != want).any(axis=2).sum()))
    # independent of --samples: the same AO picture at a small size, next to a supersampled beauty frame
    assert main([yml, "-w", "97", "-h", "61", "--ao", "2,8", "--samples", "2", "-o", str(tmp_path / "two.png")]) == 0
    assert sorted(p.name for p in tmp_path.glob("two*.png")) == ["two.ao.png", "two.png"]
    ref = ao_cases.ref(example_scenes, "test1", 97, 61, 2, 8.0, 1e-13)
    assert np.array_equal(png(tmp_path / "two.ao.png"), ao.visualize(ref[1]))
    assert "--ao" in construct_app().format_help()
