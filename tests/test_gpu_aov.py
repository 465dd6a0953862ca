"""AOV layers on the GPU (rg_render_aov / rg_render_aov_async; csrc/rg_aov.hip) against the AOV reference
of tests/aov_ref.py, which tests/test_aov_cpu.py ties to the pinned oracle.

The bar: `body`, `depth`, `normal` and `albedo` bit-identical to the reference; `uv` bit-identical for
planes, disks and AABBs, and within 2^-22 for spheres, whose coordinates go through atan2 / acos of two
different libms (a last-place difference of the f64 result can move the rounded f32 by one ulp, and the
two or three correctly rounded f32 operations behind it keep that to a couple of ulps in [0, 1]).  Ray
counts: primary == the pixels, the rest 0.  Frames are small (1x1, 17x3, 97x61, 160x120: partial tiles,
more than one wave and block); every reference is computed once and shared read-only.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import aov_ref
from gpu_launch import native_cli_path, png, require_device
from raingun_amd import _abi, aov
from raingun_amd.camera import Camera
from raingun_amd.color import Color
from raingun_amd.scene import AABB, DeviceScene, Material, Scene, Sphere
from test_gpu_camera import PATHS, POSES, _scene

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (17, 3), (97, 61), (160, 120)]
SCENES = ["test1", "test2", "test3", "synth16", "synth64", "slab"]
UV_TOL = 2.0 ** -22
TILINGS = ((8, 3, 1), (16, 2, 0))


@pytest.fixture(scope="module", autouse=True)
def _device():
    require_device()


def _ref(example_scenes, name, w, h, cam=None, **tiling):
    return aov_ref.cached(name, _scene(example_scenes, name), w, h, cam, **tiling)


def _assert_layers(scene, got, ref_layers, what, layers=aov.LAYERS):
    """got == the reference under the module's bar; returns the uv values that are not bit-identical."""
    uv_diff = 0
    for n in layers:
        g, r = np.asarray(got[n]), ref_layers[n]
        assert g.shape == r.shape and g.dtype == r.dtype, (what, n, g.shape, r.shape)
        same = aov_ref.bits(g) == aov_ref.bits(r)
        if n != "uv":
            assert same.all(), f"{what}: {int((~same).sum())} {n} values differ"
            continue
        uv_diff = int((~same).sum())
        body = ref_layers["body"]
        sphere = np.zeros(body.shape, bool)
        for i, b in enumerate(scene.bodies):
            if isinstance(b, Sphere):
                sphere |= body == i
        assert same[~sphere].all(), f"{what}: uv differs off the spheres"
        delta = float(np.abs(g.astype(np.float64) - r.astype(np.float64)).max()) if g.size else 0.0
        assert delta <= UV_TOL, f"{what}: uv differs by {delta}"
    return uv_diff


def _counts(st, pixels):
    assert st.rays.as_dict() == {"primary": pixels, "shadow": 0, "secondary": 0}
    assert st.error_pixel == -1


def _has_bvh(ds):
    return bool(ds.bvh_info().built)


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_parity(example_scenes, name, w, h):
    scene = _scene(example_scenes, name)
    st_ref, ref, counts, err = _ref(example_scenes, name, w, h)
    assert st_ref == 0 and err == -1 and counts["primary"] == w * h
    for path in PATHS:
        ds = DeviceScene(scene, path=path)
        try:
            for bvh in ((True, False) if _has_bvh(ds) else (None,)):
                if bvh is not None:
                    ds.set_bvh(bvh)
                st = _abi.rg_stats()
                got = ds.render_aov(w, h, stats=st)
                what = f"{name} {w}x{h} path {path} bvh {bvh}"
                n = _assert_layers(scene, got, ref, what)
                print(f"{what}: {n} uv values not bit-identical")
                _counts(st, w * h)
        finally:
            ds.close()


def test_lane_walk_flavour(example_scenes):
    """rg_debug_set_lane_depth(0): rays of every depth walk the BVH per lane, a camera's primary rays too."""
    name, w, h, cam = "synth64", 97, 61, POSES["look"]
    scene = _scene(example_scenes, name)
    ds = DeviceScene(scene, path=_abi.PATH_HEAVY)
    try:
        ds.set_lane_depth(0)
        for c in (None, cam):
            ds.set_camera(c)
            st = _abi.rg_stats()
            _assert_layers(scene, ds.render_aov(w, h, stats=st), _ref(example_scenes, name, w, h, c)[1], f"lane walk {c}")
            _counts(st, w * h)
    finally:
        ds.close()


# ---------------------------------------------------------------- camera
@pytest.mark.parametrize("name", ["test1", "test3", "synth64"])
def test_identity_camera_is_no_camera(example_scenes, name):
    w, h = 97, 61
    scene = _scene(example_scenes, name)
    for path in PATHS:
        ds = DeviceScene(scene, path=path)
        try:
            base = ds.render_aov(w, h)
            ds.set_camera(Camera.identity())
            st = _abi.rg_stats()
            with_cam = ds.render_aov(w, h, stats=st)
            _counts(st, w * h)
            for n in aov.LAYERS:
                assert np.array_equal(aov_ref.bits(with_cam[n]), aov_ref.bits(base[n])), (name, path, n)
        finally:
            ds.close()


@pytest.mark.parametrize("pose", ["look", "far"])
@pytest.mark.parametrize("name", ["test1", "synth64", "slab"])
def test_camera_poses(example_scenes, name, pose):
    w, h, cam = 97, 61, POSES[pose]
    scene = _scene(example_scenes, name)
    st_ref, ref, _, _ = _ref(example_scenes, name, w, h, cam)
    assert st_ref == 0
    for path in PATHS:
        ds = DeviceScene(scene, path=path)
        try:
            ds.set_camera(cam)
            for bvh in ((True, False) if _has_bvh(ds) else (None,)):
                if bvh is not None:
                    ds.set_bvh(bvh)
                st = _abi.rg_stats()
                n = _assert_layers(scene, ds.render_aov(w, h, stats=st), ref, f"{name} {pose} path {path} bvh {bvh}")
                print(f"{name} {pose} path {path} bvh {bvh}: {n} uv values not bit-identical")
                _counts(st, w * h)
        finally:
            ds.close()


# ---------------------------------------------------------------- tilings, streams
@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_tilings(example_scenes, name):
    import torch

    w, h, cam = 97, 61, POSES["look"]
    scene = _scene(example_scenes, name)
    ds = DeviceScene(scene)
    try:
        for c in (None, cam):
            ds.set_camera(c)
            for rows, stride, offset in TILINGS:
                st_ref, ref, counts, _ = _ref(example_scenes, name, w, h, c, tile_rows=rows, stride=stride, offset=offset)
                st = _abi.rg_stats()
                got = ds.render_aov_tiles(w, h, rows, stride, offset, stats=st)
                torch.cuda.synchronize()
                got = {n: t.cpu().numpy() for n, t in got.items()}
                _assert_layers(scene, got, ref, f"{name} tiling {rows, stride, offset} camera {c is not None}")
                assert st.rays.as_dict() == counts and st.error_pixel == -1
                if (rows, stride, offset) == (8, 3, 1):  # rows 56..63 of tile 7: 61, 62, 63 are padding
                    pad = slice(-3, None)
                    assert (got["body"][pad] == -1).all() and np.isposinf(got["depth"][pad]).all()
                    assert not got["normal"][pad].any() and not got["uv"][pad].any() and not got["albedo"][pad].any()
    finally:
        ds.close()


@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_three_cameras_in_flight(example_scenes, name):
    """Three streams, three cameras set between three rg_render_aov_async launches, no synchronisation in
    between: each stream has its own launch context and the camera travels by value."""
    import torch

    w, h = 97, 61
    cams = [POSES["look"], POSES["down"], POSES["sheared"]]
    scene = _scene(example_scenes, name)
    refs = [_ref(example_scenes, name, w, h, c) for c in cams]
    ds = DeviceScene(scene)
    streams = [torch.cuda.Stream() for _ in cams]
    try:
        for rounds in range(2):  # the second round finds every stream's launch context in place
            outs = []
            for cam, s in zip(cams, streams):
                ds.set_camera(cam)
                outs.append(ds.render_aov_tiles(w, h, stream=s.cuda_stream))
            ds.set_camera(None)
            torch.cuda.synchronize()
            for k, (out, s) in enumerate(zip(outs, streams)):
                got = {n: t.cpu().numpy() for n, t in out.items()}
                _assert_layers(scene, got, refs[k][1], f"{name} stream {k} round {rounds}")
                assert ds.stream_status(s.cuda_stream) == (_abi.RG_OK, -1)
        # a beauty frame on one of the streams afterwards finds its counter set zeroed
        st = _abi.rg_stats()
        t = _abi.rg_tiling(h, 1, 0)
        rgba = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
        _abi.check(_abi.lib().rg_render_tiles_async(ds.handle, w, h, C.byref(t), C.c_void_p(rgba.data_ptr()), None,
                                                    C.c_void_p(streams[0].cuda_stream), C.byref(st)))
        assert st.rays.primary == w * h and st.error_pixel == -1
        st2 = _abi.rg_stats()
        ds.render_aov_tiles(w, h, stream=streams[0].cuda_stream, stats=st2)
        _counts(st2, w * h)
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
    scene = _scene(example_scenes, name)
    _, ref, counts, _ = _ref(example_scenes, name, w, h)
    ds = DeviceScene(scene)
    stream = torch.cuda.Stream()
    hs = stream.cuda_stream
    try:
        def frame(what):
            st = _abi.rg_stats()
            got = ds.render_aov_tiles(w, h, stream=hs, stats=st)
            stream.synchronize()
            _assert_layers(scene, {n: t.cpu().numpy() for n, t in got.items()}, ref, what)
            assert st.rays.as_dict() == counts and st.error_pixel == -1, what

        frame("the frame before")  # its counts stay in the set the next launch zeroes
        big = torch.full((5 * 4096,), CANARY, dtype=torch.uint8, device="cuda")
        v = _abi.rg_aov(**{n: big.data_ptr() + 4096 * i for i, n in enumerate(aov.LAYERS)})
        t = _abi.rg_tiling(8, 2, 1)
        assert _abi.lib().rg_tiling_rows(h, C.byref(t)) == 0
        st = _abi.rg_stats()
        st.rays.primary, st.error_pixel = 77, 5
        status = _abi.lib().rg_render_aov_async(ds.handle, w, h, C.byref(t), C.byref(v), C.c_void_p(hs),
                                                C.byref(st) if with_stats else None)
        assert status == _abi.RG_OK
        if with_stats:
            assert st.rays.as_dict() == {"primary": 0, "shadow": 0, "secondary": 0} and st.error_pixel == -1
        frame("the frame after")
        assert bool((big == CANARY).all()), "a store under a tiling that selects nothing"
        assert ds.stream_status(hs) == (_abi.RG_OK, -1)
    finally:
        ds.release_stream(hs)
        ds.close()


# ---------------------------------------------------------------- layer subsets
SUBSETS =[(n,) for n in aov.LAYERS] + [("body", "depth")]
CANARY = 0xA5


@pytest.mark.parametrize("layers", SUBSETS, ids=["+".join(s) for s in SUBSETS])
def test_layer_subsets_store_nothing_else(example_scenes, layers):
    """Every layer's buffer lies in one canary-filled allocation, guards between them; only the requested
    layers' pointers are passed, and afterwards every other byte still holds the canary."""
    import torch

    name, w, h = "test1", 97, 61
    scene = _scene(example_scenes, name)
    ref = _ref(example_scenes, name, w, h)[1]
    guard = 4096
    sizes = {n: int(np.prod(aov.layer_shape(n, h, w))) * np.dtype(aov.DTYPES[n]).itemsize for n in aov.LAYERS}
    offs, total = {}, guard
    for n in aov.LAYERS:
        offs[n] = total
        total += (sizes[n] + guard + 255) // 256 * 256
    for path in PATHS:
        ds = DeviceScene(scene, path=path)
        try:
            big = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
            v = _abi.rg_aov(**{n: big.data_ptr() + offs[n] for n in layers})
            t = _abi.rg_tiling(h, 1, 0)
            st = _abi.rg_stats()
            _abi.check(_abi.lib().rg_render_aov_async(ds.handle, w, h, C.byref(t), C.byref(v), None, C.byref(st)))
            _counts(st, w * h)
            host = big.cpu().numpy()
            got = {}
            for n in layers:
                raw = host[offs[n]:offs[n] + sizes[n]]
                got[n] = raw.view(aov.DTYPES[n]).reshape(aov.layer_shape(n, h, w))
            checked = {**ref, **got}  # _assert_layers reads the reference's body for the sphere mask
            _assert_layers(scene, checked, ref, f"subset {layers} path {path}", layers)
            untouched = np.ones(total, bool)
            for n in layers:
                untouched[offs[n]:offs[n] + sizes[n]] = False
            assert (host[untouched] == CANARY).all(), f"subset {layers} path {path}: a store outside the requested layers"
        finally:
            ds.close()


# ---------------------------------------------------------------- rg_trace
@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_body_and_depth_are_rg_trace(oracle_lib, example_scenes, name):
    w, h = 97, 61
    scene = _scene(example_scenes, name)
    rays = aov_ref.prime_rays(scene.fov, w, h, oracle_lib.lib().rgo_fov_adjustment(scene.fov))
    for path in PATHS:
        ds = DeviceScene(scene, path=path)
        try:
            dist, body = ds.trace(rays)
            got = ds.render_aov(w, h, ("body", "depth"))
            assert np.array_equal(got["body"].ravel(), body), (name, path)
            want = np.where(body < 0, np.inf, dist)
            assert np.array_equal(aov_ref.bits(got["depth"].ravel()), aov_ref.bits(want)), (name, path)
        finally:
            ds.close()


# ---------------------------------------------------------------- errors
@pytest.mark.parametrize("path", PATHS)
def test_aabb_normal_error(path):
    """The reference's AABB-normal assert (bodies.rs:324): raised only when the normal layer is requested,
    with the reference's first pixel and that pixel's normal (1,0,0); the layers are still delivered."""
    bad = Scene(bodies=[AABB(((-3e8, -3e8, -7e8), (3e8, 3e8, -5e8)), Material(Color.from_str("#ffffff"), 0.5))])
    w, h = 64, 48
    for cam in (None, Camera.look_at((1e8, 2e8, 3e8), (0.0, 0.0, -6e8))):
        r_st, ref, _, r_err = aov_ref.render(bad, w, h, cam)
        assert r_st == _abi.RG_ERR_AABB_NORMAL and r_err >= 0
        ds = DeviceScene(bad, path=path)
        try:
            ds.set_camera(cam)
            out = {n: np.zeros(aov.layer_shape(n, h, w), aov.DTYPES[n]) for n in aov.LAYERS}
            st = _abi.rg_stats()
            v = _abi.rg_aov(**{n: a.ctypes.data for n, a in out.items()})
            assert _abi.lib().rg_render_aov(ds.handle, w, h, C.byref(v), C.byref(st)) == r_st
            assert st.error_pixel == r_err and st.rays.primary == w * h
            _assert_layers(bad, out, ref, f"aabb normal path {path}")
            assert tuple(out["normal"].reshape(-1, 3)[r_err]) == (1.0, 0.0, 0.0)
            st = _abi.rg_stats()
            rest = ds.render_aov(w, h, ("body", "depth", "uv", "albedo"), stats=st)  # RG_OK: no exception
            _counts(st, w * h)
            _assert_layers(bad, rest, ref, f"aabb without the normal, path {path}", ("body", "depth", "uv", "albedo"))
        finally:
            ds.close()


def test_rejections(example_scenes):
    import torch

    lib = _abi.lib()
    INVALID = _abi.RG_ERR_INVALID_ARGUMENT
    ds = DeviceScene(example_scenes["test2"])
    try:
        buf = np.full(64 * 48, 7.0)
        some, none = _abi.rg_aov(depth=buf.ctypes.data), _abi.rg_aov()
        dbuf = torch.full((64 * 48,), 7.0, dtype=torch.float64, device="cuda")
        dsome = _abi.rg_aov(depth=dbuf.data_ptr())
        t = _abi.rg_tiling(48, 1, 0)
        assert lib.rg_render_aov(ds.handle, 48, 64, C.byref(some), None) == _abi.RG_ERR_PORTRAIT
        assert lib.rg_render_aov(ds.handle, 64, 48, None, None) == INVALID
        assert lib.rg_render_aov(ds.handle, 64, 48, C.byref(none), None) == INVALID
        assert lib.rg_render_aov(ds.handle, 0, 48, C.byref(some), None) == INVALID
        assert lib.rg_render_aov(ds.handle, 1 << 16, 1 << 16, C.byref(some), None) == INVALID
        assert lib.rg_render_aov(None, 64, 48, C.byref(some), None) == INVALID
        assert lib.rg_render_aov_async(ds.handle, 48, 64, C.byref(t), C.byref(dsome), None, None) == _abi.RG_ERR_PORTRAIT
        assert lib.rg_render_aov_async(ds.handle, 64, 48, C.byref(t), None, None, None) == INVALID
        assert lib.rg_render_aov_async(ds.handle, 64, 48, C.byref(t), C.byref(none), None, None) == INVALID
        assert lib.rg_render_aov_async(ds.handle, 64, 48, None, C.byref(dsome), None, None) == INVALID
        for bad in (_abi.rg_tiling(0, 1, 0), _abi.rg_tiling(8, 0, 0), _abi.rg_tiling(8, 2, 2)):
            assert lib.rg_render_aov_async(ds.handle, 64, 48, C.byref(bad), C.byref(dsome), None, None) == INVALID
        torch.cuda.synchronize()
        assert (buf == 7.0).all() and bool((dbuf == 7.0).all())  # a rejected call writes nothing
        with pytest.raises(ValueError):
            ds.render_aov(64, 48, ("beauty",))
    finally:
        ds.close()


# ---------------------------------------------------------------- both command lines
def _check_cli_outputs(example_scenes, tmp_path, stem, plain):
    w, h = 800, 600  # --draft
    cam = Camera.look_at((3, 2, -10), (0, 0, -30))
    ref = _ref(example_scenes, "test1", w, h, cam)[1]
    for n in aov.LAYERS:
        got = png(tmp_path / f"{stem}.{n}.png")
        want = aov.visualize(n, ref[n])
        assert np.array_equal(got, want), (n, int((got != want).any(axis=2).sum()))
    assert (tmp_path / f"{stem}.png").read_bytes() == plain.read_bytes()


CLI_FLAGS = ["--draft", "--eye", "3,2,-10", "--look-at=0,0,-30"]


def test_native_cli_aov(example_scenes, golden_dir, tmp_path):
    cli, yml = native_cli_path(), str(golden_dir / "examples" / "test1.yml")
    plain = tmp_path / "plain.png"
    for flags, out in (([], plain), (["--aov", "all"], tmp_path / "cli.png")):
        r = subprocess.run([cli, *CLI_FLAGS, *flags, "-o", str(out), yml], cwd=golden_dir, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
    assert not list(tmp_path.glob("plain.*.png"))
    _check_cli_outputs(example_scenes, tmp_path, "cli", plain)
    bad_width = subprocess.run([cli, "--samples", "9", yml], capture_output=True, text=True, timeout=60)
    for flags in (["--aov", "beauty"], ["--aov", "body,"], ["--aov", ""], ["--aov"]):
        r = subprocess.run([cli, *flags, "-o", str(tmp_path / "no.png"), yml], capture_output=True, text=True, timeout=60)
        assert r.returncode == bad_width.returncode == 1 and r.stderr.startswith("error:"), (flags, r.returncode, r.stderr)
    assert not list(tmp_path.glob("no*.png"))


def test_python_cli_aov(example_scenes, golden_dir, tmp_path, monkeypatch):
    from raingun_amd.cli import main

    monkeypatch.chdir(golden_dir)  # textures resolve against the working directory
    yml = str(golden_dir / "examples" / "test1.yml")
    plain = tmp_path / "plain.png"
    assert main([yml, *CLI_FLAGS, "-o", str(plain)]) == 0
    assert main([yml, *CLI_FLAGS, "--aov", "all", "-o", str(tmp_path / "py.png")]) == 0
    _check_cli_outputs(example_scenes, tmp_path, "py", plain)
    assert main([yml, "-w", "97", "-h", "61", "--aov", "depth,body", "--samples", "2", "-o", str(tmp_path / "two.png")]) == 0
    assert sorted(p.name for p in tmp_path.glob("two*.png")) == ["two.body.png", "two.depth.png", "two.png"]
    ref = _ref(example_scenes, "test1", 97, 61)[1]
    for n in ("body", "depth"):  # one ray per pixel whatever --samples says
        assert np.array_equal(png(tmp_path / f"two.{n}.png"), aov.visualize(n, ref[n]))
