"""The host-facing entry points of the C ABI against the CPU restatement:
host-visible frames (rg_render_image: by default ONE launch whose pixel stores
go over PCIe into page-locked memory -- the caller's, or a pinned frame whose
published tiles are copied into a pageable caller buffer band by band while
the kernel renders on; forced banded renders with device-to-host copies),
tile streaming from one launch (rg_render_stream), the single-process multi-GPU entry
(rg_render_multi), recursion deeper than the compiled frame arrays, and the
reference's panic sites as status codes (scene.rs:38 NaN distance for
closest-hit AND shadow rays, rendering.rs:106 transmission, bodies.rs:324
AABB normal) -- status and first pixel equal to the restatement's.
"""
import ctypes as C
import time

import numpy as np
import pytest

from gpu_launch import require_device
from raingun_amd import _abi
from raingun_amd.color import Color
from raingun_amd.scene import (AABB, DeviceScene, DirectionalLight, Material, Plane, Scene, SceneDesc, Sphere,
                               SphericalLight)
from raingun_amd.synth import synthetic_scene

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4
WHITE = Color.from_str("#ffffff")


@pytest.fixture(scope="module", autouse=True)
def _device():
    require_device()


def _oracle(oracle_lib, scene, w, h):
    st, rgba, rgb, counts, err = oracle_lib.render(SceneDesc(scene), w, h, want_rgb=True)
    return st, rgba, rgb, counts, err


# ---------------------------------------------------------------- host-visible frames
@pytest.mark.parametrize("bands", [-2, -1, 0, 1, 3, 7])  # -1: one launch writing host memory; -2 split; 0: automatic
@pytest.mark.parametrize("kind,w,h", [("test1", 800, 600), ("synth200", 640, 360), ("test2", 97, 61),
                                      ("test3", 33, 9)])
@pytest.mark.parametrize("pinned", [False, True])
def test_render_image_host_visible(oracle_lib, example_scenes, kind, w, h, bands, pinned):
    scene = synthetic_scene(200, 2, 5) if kind == "synth200" else example_scenes[kind]
    o_st, o_rgba, _, o_counts, _ = _oracle(oracle_lib, scene, w, h)
    assert o_st == 0
    ds = DeviceScene(scene)
    ds.set_image_bands(bands)
    out = np.full((h, w, 4), 123, dtype=np.uint8)
    reg = _abi.HostRegistration(out) if pinned else None
    try:
        for _ in range(2):  # the scene's framebuffer / staging are reused across calls
            st = _abi.rg_stats()
            got = ds.render_image(w, h, stats=st, out=out)
            assert np.array_equal(got, o_rgba)
            assert st.rays.as_dict() == o_counts
            assert st.error_pixel == -1
    finally:
        if reg is not None:
            reg.close()
        ds.close()


@pytest.mark.parametrize("depth", [5, 8, 9, 66])  # <= 8 frames: array-frame host kernels (HF); deeper: MAXD == 0
@pytest.mark.parametrize("bands", [-2, -1, 0])
@pytest.mark.parametrize("pinned", [False, True])
def test_heavy_host_frames_by_depth(oracle_lib, depth, bands, pinned):
    """Host-visible frames of a heavy-path (BVH) scene on both host-frame kernel
    families: scenes needing at most 8 frames run the MAXD = 8 array-frame kernels
    with the host-frame features, deeper ones the MAXD = 0 kernels (rg_kernels.hip
    dispatch_depth); the automatic 16x4 host tiles in both."""
    scene = synthetic_scene(200, 2, 5) if depth <= 9 else _mirror_corridor(depth)
    scene.max_recursion_depth = depth
    w, h = 160, 90
    o_st, o_rgba, _, o_counts, _ = _oracle(oracle_lib, scene, w, h)
    assert o_st == 0
    ds = DeviceScene(scene, path=_abi.PATH_HEAVY)
    ds.set_image_bands(bands)
    out = np.full((h, w, 4), 77, dtype=np.uint8)
    reg = _abi.HostRegistration(out) if pinned else None
    try:
        for _ in range(2):
            st = _abi.rg_stats()
            got = ds.render_image(w, h, stats=st, out=out)
            assert np.array_equal(got, o_rgba)
            assert st.rays.as_dict() == o_counts
    finally:
        if reg is not None:
            reg.close()
        ds.close()


@pytest.mark.parametrize("wlog", [0, 3, 4, 5, 6])  # 0: the automatic shape
@pytest.mark.parametrize("kind,w,h", [("test1", 321, 243), ("synth200", 200, 111), ("test3", 97, 61)])
def test_host_tile_shapes(oracle_lib, example_scenes, kind, w, h, wlog):
    """One-launch host-visible frames with every tile shape (8x8 .. 64x1; the
    tile probe and ordering, partial tiles at the right and bottom edges, the
    band bookkeeping of the pageable copy) against the CPU restatement."""
    scene = synthetic_scene(200, 2, 5) if kind == "synth200" else example_scenes[kind]
    o_st, o_rgba, _, o_counts, _ = _oracle(oracle_lib, scene, w, h)
    assert o_st == 0
    ds = DeviceScene(scene)
    ds.set_image_bands(-1)
    ds.set_host_tile_shape(wlog)
    for pinned in (False, True):
        out = np.full((h, w, 4), 7, dtype=np.uint8)
        reg = _abi.HostRegistration(out) if pinned else None
        try:
            st = _abi.rg_stats()
            ds.render_image(w, h, stats=st, out=out)
            assert np.array_equal(out, o_rgba)
            assert st.rays.as_dict() == o_counts
        finally:
            if reg is not None:
                reg.close()
    got = np.zeros_like(o_rgba)
    _abi.check(ds.render_stream(w, h, lambda r, b: got.__setitem__(slice(r, r + b.shape[0]), b), 13))
    assert np.array_equal(got, o_rgba)
    ds.close()


@pytest.mark.parametrize("kind,w,h", [("test1", 3840, 2160), ("synth200", 640, 360)])
@pytest.mark.parametrize("pinned", [False, True])
def test_render_image_direct_many_frames(oracle_lib, example_scenes, kind, w, h, pinned):
    """The tile-publication protocol under load: 40 back-to-back frames into
    the same host buffer (poisoned between calls) -- test1 at 4K (light path)
    and a 200-sphere scene small enough for the heavy path's task splitting;
    every frame equals the CPU restatement's, byte for byte (a tile copied
    before its pixels landed would show)."""
    import copy

    if kind == "synth200":
        s = synthetic_scene(200, 2, 5)
    else:
        s = copy.copy(example_scenes["test1"])
        s.max_recursion_depth = 5
    o_st, ref, _, _, _ = _oracle(oracle_lib, s, w, h)
    assert o_st == 0
    ds = DeviceScene(s)
    ds.set_image_bands(-1)
    out = np.empty((h, w, 4), dtype=np.uint8)
    reg = _abi.HostRegistration(out) if pinned else None
    try:
        for k in range(40):
            out.fill(k & 0xFF)
            ds.render_image(w, h, out=out)
            assert np.array_equal(out, ref), k
    finally:
        if reg is not None:
            reg.close()
        ds.close()


def test_split_frame_error_exit_leaves_no_writer(example_scenes):
    """the split host path (part B, a kernel storing into the caller's page-locked
    frame, enqueued first) must not return while anything still writes that frame.  Part A's launch
    is made to fail once (rg_debug_fail_split_a): the call returns RG_ERR_DEVICE, and at that moment
    every row is either untouched (part A's, sentinel) or already final (part B's); nothing changes
    afterwards; the next call renders the whole frame again."""
    import copy
    import time

    s = copy.copy(example_scenes["test1"])
    s.max_recursion_depth = 5
    w, h = 3840, 2160
    ds = DeviceScene(s)
    ds.set_image_bands(-2)
    ref = ds.render_image(w, h)
    out = np.empty((h, w, 4), dtype=np.uint8)
    reg = _abi.HostRegistration(out)
    try:
        out.fill(0xAB)
        _abi.check(_abi.lib().rg_debug_fail_split_a(ds.handle, 1))
        st = _abi.lib().rg_render_image(ds.handle, w, h, out.ctypes.data, None)
        snap = out.copy()
        assert st == _abi.RG_ERR_DEVICE
        untouched = (snap == 0xAB).all(axis=(1, 2))
        final = (snap == ref).all(axis=(1, 2))
        assert (untouched | final).all(), np.flatnonzero(~(untouched | final))[:8]
        assert final[-1] and untouched[0] and final.sum() > h // 2  # part B (the bottom ~65 %) ran to the end
        time.sleep(0.2)
        assert np.array_equal(out, snap)  # no kernel or DMA wrote the buffer after the call returned
        ds.render_image(w, h, out=out)  # the injected failure does not stick
        assert np.array_equal(out, ref)
    finally:
        reg.close()
        ds.close()


def test_render_image_4k_default_bands(oracle_lib, example_scenes):
    """BASELINE configs[1] through the drop-in itself: test1 3840x2160 depth 5,
    host-visible, the library's default band count."""
    import copy

    s = copy.copy(example_scenes["test1"])
    s.max_recursion_depth = 5
    o_st, o_rgba, _, o_counts, _ = _oracle(oracle_lib, s, 3840, 2160)
    ds = DeviceScene(s)
    st = _abi.rg_stats()
    got = ds.render_image(3840, 2160, stats=st)
    ds.close()
    assert np.array_equal(got, o_rgba)
    assert st.rays.as_dict() == o_counts


@pytest.mark.parametrize("tile_rows,stride,offset", [(8, 3, 1), (600, 1, 0), (7, 1, 0), (5, 2, 1)])
def test_render_tiles_rgb_host(oracle_lib, example_scenes, tile_rows, stride, offset):
    """rg_render_tiles (host buffers, f32 RGB too): a whole-frame tiling is
    banded, a sharded one is one launch; padding rows come back zeroed."""
    s = example_scenes["test1"]
    w, h = 320, 243
    ds = DeviceScene(s)
    ds.set_image_bands(3)
    rgba, rgb = ds.render_tiles(w, h, tile_rows, stride, offset, want_rgb=True)
    ds.close()
    o_st, o_rgba, o_rgb, _, _ = oracle_lib.render(SceneDesc(s), w, h, tile_rows, stride, offset, want_rgb=True)
    assert o_st == 0
    assert np.array_equal(rgba, o_rgba)
    assert float(np.abs(rgb - o_rgb).max()) <= RGB_TOL


def test_banded_and_supersampled_frames_interleaved(oracle_lib, example_scenes):
    """Host-visible and supersampled frames of one scene in turn, into pageable memory: each kind
    has band resources of its own (streams, events, device frame, staging ring), grown on demand
    -- 1, then 16 bands of 8 rows (more than staging slots), then fewer again; supersampled bands
    of 7 rows between them; then both at other sizes, with the f32 output.  Every frame equals the
    CPU restatement's byte for byte (supersampled: the restatement at k w x k h, box-filtered in
    numpy), ray counts equal."""
    from raingun_amd import aa

    scene = example_scenes["test1"]

    def image(ds, w, h, bands):
        o_st, o_rgba, _, o_counts, _ = _oracle(oracle_lib, scene, w, h)
        assert o_st == 0
        for k in bands:
            ds.set_image_bands(k)
            st = _abi.rg_stats()
            got = ds.render_image(w, h, stats=st, out=np.full((h, w, 4), 123, dtype=np.uint8))
            assert np.array_equal(got, o_rgba), f"{w}x{h}, {k} bands"
            assert st.rays.as_dict() == o_counts, f"{w}x{h}, {k} bands"
            assert st.error_pixel == -1

    def supersampled(ds, w, h, k, band_rows, want_rgb):
        o_st, _, o_rgb, o_counts, _ = _oracle(oracle_lib, scene, k * w, k * h)
        assert o_st == 0
        want_mean, want_rgba = aa.resolve_box(o_rgb, k)
        ds.set_aa_band_rows(band_rows)
        st = _abi.rg_stats()
        got = ds.render_image_aa(w, h, k, want_rgb=want_rgb, stats=st)
        rgba, mean = got if want_rgb else (got, None)
        assert np.array_equal(rgba, want_rgba), f"{w}x{h} k {k}"
        if want_rgb:
            assert float(np.abs(mean.astype(np.float64) - want_mean.astype(np.float64)).max()) <= RGB_TOL
        assert st.rays.as_dict() == o_counts, f"{w}x{h} k {k}"
        assert st.error_pixel == -1

    ds = DeviceScene(scene)
    try:
        image(ds, 160, 128, (1, 16, 3))
        supersampled(ds, 64, 40, 2, 7, False)  # 6 bands
        image(ds, 97, 61, (7,))                # 4 bands of 16 rows, the last one short
        supersampled(ds, 101, 75, 3, 16, True)
    finally:
        ds.close()


# ---------------------------------------------------------------- streaming
@pytest.mark.parametrize("tile_rows", [32, 37, 240, 1])
def test_stream_bands_match_oracle(oracle_lib, example_scenes, tile_rows):
    """render_image_stream (rendering.rs:40-69) as tile callbacks: every band
    equals the CPU restatement's rows; one launch renders on while a slow
    callback holds a band (the bands still arrive in order, complete)."""
    s = example_scenes["test1"]
    w, h = 320, 240
    o_st, o_rgba, _, o_counts, _ = _oracle(oracle_lib, s, w, h)
    got = np.zeros_like(o_rgba)
    seen = []

    def on_tile(row0, band):
        if len(seen) < 4:
            time.sleep(0.002)
        got[row0:row0 + band.shape[0]] = band
        seen.append((row0, band.shape[0]))
        return False

    ds = DeviceScene(s)
    st = _abi.rg_stats()
    _abi.check(ds.render_stream(w, h, on_tile, tile_rows, st))
    ds.close()
    assert np.array_equal(got, o_rgba)
    assert [r for r, _ in seen] == list(range(0, h, tile_rows))
    assert sum(n for _, n in seen) == h
    assert st.rays.as_dict() == o_counts


def test_stream_cancel_after_two_bands(example_scenes):
    s = example_scenes["test2"]
    calls = []
    ds = DeviceScene(s)
    status = ds.render_stream(320, 240, lambda r, b: calls.append(r) or len(calls) == 2, 32)
    # the scene stays usable after a cancelled stream
    full = ds.render_image(320, 240)
    ds.close()
    assert status == _abi.RG_ERR_CANCELLED
    assert calls == [0, 32]
    assert full.shape == (240, 320, 4)


# ---------------------------------------------------------------- panic sites
def _far_sphere_scene(fov, with_ceiling=True):
    """A sphere at 5e154: for a ray whose direction has a large component along
    it, h.h and adj^2 both overflow and opp = inf - inf is NaN (bodies.rs:95),
    so the sphere 'hits' at NaN.  Scene::trace panics (scene.rs:38) when a ray
    has another hit besides.  fov 90: the primary rays of the top rows already
    do; fov 30: only the shadow rays towards the light overhead do."""
    m = Material(WHITE, 0.5)
    bodies = [Sphere((0.0, 5e154, 0.0), 1.0, m), Plane((0.0, -2.0, 0.0), (0.0, -1.0, 0.0), m)]
    if with_ceiling:
        bodies.append(Plane((0.0, 10.0, 0.0), (0.0, 1.0, 0.0), m))
    return Scene(fov=fov, bodies=bodies, lights=[DirectionalLight((0.0, -1.0, 0.0), WHITE, 1.0)])


def _error_case(oracle_lib, scene, w, h, path):
    o_st, o_rgba, _, o_counts, o_err = _oracle(oracle_lib, scene, w, h)
    ds = DeviceScene(scene, path=path)
    st = _abi.rg_stats()
    out = np.zeros((h, w, 4), np.uint8)
    status = _abi.lib().rg_render_image(ds.handle, w, h, out.ctypes.data, C.byref(st))
    ds.close()
    assert status == o_st, (status, o_st)
    assert st.error_pixel == o_err
    assert st.rays.as_dict() == o_counts
    assert np.array_equal(out, o_rgba)  # the frame is delivered either way
    return status


PATHS = [_abi.PATH_LIGHT, _abi.PATH_HEAVY]


@pytest.mark.parametrize("path", PATHS)
def test_nan_distance_closest_hit(oracle_lib, path):
    assert _error_case(oracle_lib, _far_sphere_scene(90.0), 5, 3, path) == _abi.RG_ERR_NAN_DISTANCE


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("w,h", [(5, 3), (64, 36)])
def test_nan_distance_shadow_ray(oracle_lib, path, w, h):
    """Primary rays see no NaN (fov 30); shadow rays towards the overhead light
    see the NaN sphere and the ceiling: the reference panics in shade_diffuse's
    trace (rendering.rs:150 -> scene.rs:38)."""
    scene = _far_sphere_scene(30.0)
    # the primary rays alone do not panic
    rays = []
    import oracle

    fa = oracle.lib().rgo_fov_adjustment(30.0)
    for y in range(h):
        for x in range(w):
            d = np.array([(((x + 0.5) / w) * 2 - 1) * (w / h) * fa, (1 - ((y + 0.5) / h) * 2) * fa, -1.0])
            rays.append([0.0, 0.0, 0.0, *(d / np.linalg.norm(d))])
    assert oracle_lib.trace(SceneDesc(scene), np.array(rays))[0] == 0
    assert _error_case(oracle_lib, scene, w, h, path) == _abi.RG_ERR_NAN_DISTANCE


@pytest.mark.parametrize("path", PATHS)
def test_nan_distance_single_hit_shadow_is_occluded(oracle_lib, path):
    """A shadow ray whose only hit is at NaN: min_by compares nothing, no panic,
    and `dist > light distance` is false -> in shadow (rendering.rs:152-155)."""
    assert _error_case(oracle_lib, _far_sphere_scene(30.0, with_ceiling=False), 16, 9, path) == _abi.RG_OK


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("w,h", [(33, 21), (65, 37)])
def test_rays_in_aabb_slab_planes(oracle_lib, path, w, h):
    """Rays lying exactly in a slab plane of a box (d_k == 0 and o_k on the
    face: 0 * inf = NaN inside the slab test, bodies.rs:242-282).  The NaN
    never reaches Scene::trace: a NaN tmin/tmax loses every comparison and the
    test returns only tmin >= 0 or tmax >= 0, so these rays hit or miss like
    the reference and nothing panics.  The odd width puts the middle column's
    primary rays at d.x == 0 on the box face x = 0; their floor hits have
    x == 0 exactly, so the shadow rays towards the overhead light (d = (0,1,0))
    run inside the same face plane (and inside z-face planes: d.z == 0)."""
    m = Material(WHITE, 0.5)
    scene = Scene(bodies=[AABB(((0.0, -1.0, -5.0), (1.0, 1.0, -3.0)), m),
                          AABB(((-2.0, -1.5, -4.0), (0.0, -1.0, -2.5)), Material(Color.from_str("#ff8040"), 0.4)),
                          Plane((0.0, -2.0, 0.0), (0.0, -1.0, 0.0), m)],
                  lights=[DirectionalLight((0.0, -1.0, 0.0), WHITE, 1.0),
                          SphericalLight((0.0, 3.0, -4.0), WHITE, 300.0)])
    assert _error_case(oracle_lib, scene, w, h, path) == _abi.RG_OK
    # the closest-hit query itself on rays in slab planes: faces, edges, corners, both signs of zero
    rays = []
    for o in [(0.0, -2.0, -4.0), (0.0, 0.0, 0.0), (1.0, -1.0, -3.0), (0.0, -1.0, -5.0), (-2.0, -1.5, -2.5),
              (0.5, 1.0, -4.0), (0.0, 0.5, -3.0)]:
        for d in [(0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (-0.0, 1.0, 0.0), (0.0, 0.0, -1.0), (0.0, 0.0, 1.0),
                  (1.0, 0.0, 0.0), (-1.0, 0.0, -0.0), (0.6, 0.0, -0.8), (0.0, 0.6, -0.8)]:
            rays.append([*o, *d])
    rays = np.array(rays)
    o_st, o_dist, o_body = oracle_lib.trace(SceneDesc(scene), rays)
    assert o_st == 0
    ds = DeviceScene(scene, path=path)
    dist, body = ds.trace(rays)
    ds.close()
    assert np.array_equal(body, o_body)
    hit = o_body >= 0
    assert np.array_equal(dist[hit], o_dist[hit])


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("w,h", [(5, 3), (33, 21)])
def test_transmission_none_while_kr_below_one(oracle_lib, path, w, h):
    """An odd width puts a primary ray at d.x == 0 exactly; it hits the +z face
    of a refractive box whose -x face is 5e-9 from x = 0, so the face search
    (bodies.rs:311-327) returns the -x normal and i.n == 0: fresnel sees the
    outside (kr < 1), create_transmission the inside with k < 0 -> None ->
    unwrap panics (rendering.rs:106)."""
    glass = Material(WHITE, 0.5, "Refractive", 0.0, 1.5, 0.8)
    m = Material(WHITE, 0.5)
    scene = Scene(bodies=[AABB(((-5e-9, -1.0, -5.0), (1.0, 1.0, -3.0)), glass),
                          Plane((0.0, -2.0, 0.0), (0.0, -1.0, 0.0), m)],
                  lights=[DirectionalLight((0.0, -1.0, 0.0), WHITE, 1.0)])
    assert _error_case(oracle_lib, scene, w, h, path) == _abi.RG_ERR_TRANSMISSION


def test_aabb_normal_error_through_stream_status():
    """Asynchronous launches report nothing themselves; rg_stream_status returns
    the first error any launch on the stream raised, then clears it."""
    import torch

    m = Material(WHITE, 0.5)
    bad = Scene(bodies=[AABB(((-3e8, -3e8, -7e8), (3e8, 3e8, -5e8)), m)])
    ds = DeviceScene(bad)
    lib = _abi.lib()
    stream = torch.cuda.Stream()
    buf = torch.empty((48, 64, 4), dtype=torch.uint8, device="cuda")
    t = _abi.rg_tiling(48, 1, 0)
    for _ in range(3):
        _abi.check(lib.rg_render_tiles_async(ds.handle, 64, 48, C.byref(t), C.c_void_p(buf.data_ptr()), None,
                                             C.c_void_p(stream.cuda_stream), None))
    status, pixel = ds.stream_status(stream.cuda_stream)
    assert status == _abi.RG_ERR_AABB_NORMAL and pixel >= 0
    assert ds.stream_status(stream.cuda_stream) == (_abi.RG_OK, -1)  # cleared
    ds.release_stream(stream.cuda_stream)
    ds.close()


# ---------------------------------------------------------------- deep recursion
def _mirror_corridor(depth):
    """Two facing one-sided reflecting planes (behind and in front of the
    camera): every primary ray bounces until max_recursion_depth."""
    mirror = Material(Color.from_str("#a0c0ff"), 0.6, "Reflecting", 0.9)
    ball = Material(Color.from_str("#ff8040"), 0.5, "Reflecting", 0.3)
    return Scene(max_recursion_depth=depth,
                 bodies=[Plane((0.0, 0.0, -10.0), (0.0, 0.0, -1.0), mirror),
                         Plane((0.0, 0.0, 10.0), (0.0, 0.0, 1.0), mirror),
                         Sphere((1.0, 0.5, -6.0), 1.0, ball),
                         Plane((0.0, -3.0, 0.0), (0.0, -1.0, 0.0), Material(WHITE, 0.4))],
                 lights=[SphericalLight((0.0, 4.0, 0.0), WHITE, 400.0),
                         DirectionalLight((0.3, -1.0, -0.2), WHITE, 0.5)])


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("depth", [66, 100, 300])
def test_recursion_deeper_than_compiled_frames(oracle_lib, path, depth):
    """scene.rs:16 is a u32 and rendering.rs:122-130 recurses until it: depths
    above 65 keep their shading frames in device memory (FrameStack<0>)."""
    scene = _mirror_corridor(depth)
    w, h = 64, 36
    o_st, o_rgba, o_rgb, o_counts, _ = _oracle(oracle_lib, scene, w, h)
    assert o_st == 0
    assert o_counts["secondary"] >= w * h * (depth - 1) // 3  # the chains really are deep
    ds = DeviceScene(scene, path=path)
    st = _abi.rg_stats()
    rgba, rgb = ds.render_tiles(w, h, want_rgb=True, stats=st)
    ds.close()
    assert st.rays.as_dict() == o_counts
    assert np.array_equal(rgba, o_rgba)
    assert float(np.abs(rgb - o_rgb).max()) <= RGB_TOL


@pytest.mark.parametrize("path", PATHS)
def test_recursion_depth_20000_grid_capped(oracle_lib, path):
    """at depth 20000 a full persistent grid's frames (88 B x 19999 per
    thread) would need 230-350 GB; the launch caps the grid at half the free device
    memory (<= 16 GiB of frames) and the frame renders, equal to the restatement."""
    scene = _mirror_corridor(20000)
    w, h = 16, 9
    o_st, o_rgba, o_rgb, o_counts, _ = _oracle(oracle_lib, scene, w, h)
    assert o_st == 0
    assert o_counts["secondary"] > w * h * 5000
    ds = DeviceScene(scene, path=path)
    st = _abi.rg_stats()
    rgba, rgb = ds.render_tiles(w, h, want_rgb=True, stats=st)
    ds.close()
    assert st.rays.as_dict() == o_counts
    assert np.array_equal(rgba, o_rgba)
    assert float(np.abs(rgb - o_rgb).max()) <= RGB_TOL


# ---------------------------------------------------------------- rg_render_multi
@pytest.mark.parametrize("kind,w,h,tile_rows", [("test1", 320, 243, 8), ("synth200", 256, 144, 16),
                                                ("test3", 97, 61, 0)])
def test_render_multi_one_device(oracle_lib, example_scenes, kind, w, h, tile_rows):
    """The single-process multi-GPU entry at ngpus = 1: replicas, ncclCommInitAll,
    the gather to device 0 and the re-interleave all run (a 1-rank gather)."""
    import torch

    scene = synthetic_scene(200, 2, 5) if kind == "synth200" else example_scenes[kind]
    o_st, o_rgba, _, o_counts, _ = _oracle(oracle_lib, scene, w, h)
    ds = DeviceScene(scene)
    for _ in range(2):
        st = _abi.rg_stats()
        got = ds.render_multi(w, h, 1, tile_rows, stats=st)
        assert np.array_equal(got, o_rgba)
        assert st.rays.as_dict() == o_counts
    ngpu = torch.cuda.device_count()
    with pytest.raises(_abi.RaingunError) as ei:
        ds.render_multi(w, h, ngpu + 1)
    assert ei.value.status == _abi.RG_ERR_INVALID_ARGUMENT
    ds.close()


@pytest.mark.parametrize("mode", [0, 1])  # 0: per-device copies to the host; 1: gather to device 0
@pytest.mark.parametrize("ngpus,kind,w,h,T,bands", [(2, "test1", 320, 243, 8, 0), (3, "synth200", 256, 149, 16, 2),
                                                    (8, "test3", 97, 61, 8, 0), (8, "test1", 640, 357, 8, 3),
                                                    (5, "test2", 200, 77, 4, 4), (4, "synth200", 256, 149, 8, 0),
                                                    (8, "synth200", 320, 181, 8, 0), (3, "test1", 320, 243, 8, -1),
                                                    (8, "test3", 97, 61, 8, -1)])
def test_render_multi_n_devices_stand_in(oracle_lib, example_scenes, mode, ngpus, kind, w, h, T, bands):
    """VERDICT r2 item 4 / ADVICE r2: rg_render_multi at ngpus > 1 on one GPU.  Every
    "device" is this GPU with its own scene replica; mode 1's grouped gather goes
    through the library's stand-in (ncclGather's signature and group semantics), so
    the replicas, the per-device tilings, the packed-RGB parts, the root's
    re-interleave, the per-device banded copies into pageable and page-locked host
    memory, the one launch per device writing its rows straight into a page-locked
    frame (bands 0, round 4), the stats merge and heights that are not a multiple
    of the tile height all run.  Byte-exact against the CPU restatement, ray counts
    exact."""
    scene = synthetic_scene(200, 2, 5) if kind == "synth200" else example_scenes[kind]
    o_st, o_rgba, _, o_counts, _ = _oracle(oracle_lib, scene, w, h)
    assert o_st == 0
    ds = DeviceScene(scene)
    ds.set_multi(mode, stand_in=True, bands=bands)
    for pinned in (False, True):
        out = np.full((h, w, 4), 77, dtype=np.uint8)
        reg = _abi.HostRegistration(out) if pinned else None
        try:
            for _ in range(2):  # resources are kept across calls
                st = _abi.rg_stats()
                got = ds.render_multi(w, h, ngpus, T, stats=st, out=out)
                assert np.array_equal(got, o_rgba), (pinned, int((got != o_rgba).any(axis=2).sum()))
                assert st.rays.as_dict() == o_counts
                assert st.error_pixel == -1
        finally:
            if reg is not None:
                reg.close()
    ds.close()


def test_replica_follows_settings(example_scenes):
    """A replica takes every member of rg_scene_settings from its root scene before each frame
    (rg_sync_settings copies the struct whole): with the replicas made, each pixel-affecting setting is
    changed on the root scene in turn, and the two-"device" frame must equal the one-device frame byte
    for byte.  48 rows in tiles of 8 rows: three tile rows per device."""
    from raingun_amd.camera import Camera

    w, h, T = 64, 48, 8
    ds = DeviceScene(example_scenes["test1"])
    try:
        ds.set_multi(0, stand_in=True, bands=0)
        first = ds.render_multi(w, h, 2, T).copy()  # the replicas exist from here on
        assert np.array_equal(first, ds.render_image(w, h))
        # (a camera alone is also tests/test_gpu_camera.py::test_render_multi_stand_in; here it stays set
        # while the other members change)
        changes = [("max_depth 1", lambda: ds.set_max_depth(1)),
                   ("camera", lambda: ds.set_camera(Camera.look_at((3, 2, -10), (0, 0, -30)))),
                   ("path heavy", lambda: ds.set_path(_abi.PATH_HEAVY)),
                   ("bvh off", lambda: ds.set_bvh(False)),
                   ("light buffers off", lambda: ds.set_lightbuf(False)),
                   ("shadow volume off", lambda: ds.set_shadow_volume(False)),
                   ("first-hit tiles off", lambda: ds.set_first_hit_tiles(False)),
                   ("exact division off", lambda: ds.set_exact_div(False))]
        last = first
        for what, change in changes:
            change()
            st_m, st_1 = _abi.rg_stats(), _abi.rg_stats()
            multi = ds.render_multi(w, h, 2, T, stats=st_m).copy()
            one = ds.render_image(w, h, stats=st_1)
            assert np.array_equal(multi, one), (what, int((multi != one).any(axis=2).sum()))
            assert st_m.rays.as_dict() == st_1.rays.as_dict(), what
            if what in ("max_depth 1", "camera"):  # the setting took effect at all
                assert not np.array_equal(multi, last), what
            last = multi
    finally:
        ds.close()


@pytest.mark.parametrize("flush,group", [(1, 1), (2, 2), (4, 1), (8, 3), (16, 16)])
def test_light_host_ring_settings(oracle_lib, example_scenes, flush, group):
    """Round 6: the light path's LDS tile ring with a runtime flush size and queue group
    (rg_debug_set_host_ring): rg_render_multi over 8 stand-in devices, each share one launch storing
    its rows into the page-locked frame (the automatic mode for light scenes since round 6) or banded,
    and the 1-GPU split frame, whose one-launch part is a "big" launch at 4K -- byte-exact."""
    import copy

    s = copy.copy(example_scenes["test1"])
    s.max_recursion_depth = 5
    w, h = 640, 357
    o_st, o_rgba, _, o_counts, _ = _oracle(oracle_lib, s, w, h)
    ds = DeviceScene(s)
    ds.set_host_ring(flush_small=flush, group_small=group, flush_big=flush, group_big=group)
    out = np.full((h, w, 4), 77, dtype=np.uint8)
    reg = _abi.HostRegistration(out)
    try:
        for one in (1, 0):
            ds.set_host_ring(multi_light_one=one)
            ds.set_multi(0, stand_in=True, bands=0)
            st = _abi.rg_stats()
            out.fill(77)
            got = ds.render_multi(w, h, 8, 8, stats=st, out=out)
            assert np.array_equal(got, o_rgba), (one, int((got != o_rgba).any(axis=2).sum()))
            assert st.rays.as_dict() == o_counts
    finally:
        reg.close()
    ds.set_multi(0, stand_in=False, bands=0)
    W, H = 3840, 2160
    ref, _ = ds.render_tiles(W, H, want_rgb=True)  # banded device-resident path (pinned to the restatement)
    big = np.full((H, W, 4), 5, dtype=np.uint8)
    reg = _abi.HostRegistration(big)
    try:
        for _ in range(2):
            big.fill(5)
            ds.render_image(W, H, out=big)
            assert np.array_equal(big, ref)
    finally:
        reg.close()
        ds.close()


@pytest.mark.parametrize("mode,bands,pinned", [(0, 2, False), (1, 2, False), (0, -1, True), (0, 2, True)])
def test_render_multi_n_devices_reports_first_error(oracle_lib, mode, bands, pinned):
    """The NaN-distance panic (scene.rs:38) raised on several devices: the lowest
    erroring pixel over all devices (and bands) is the oracle's first pixel, the
    frame is still delivered (one launch per device into a pinned frame too)."""
    scene = _far_sphere_scene(30.0)
    o_st, o_rgba, _, o_counts, o_err = _oracle(oracle_lib, scene, 64, 36)
    assert o_st == _abi.RG_ERR_NAN_DISTANCE
    ds = DeviceScene(scene)
    ds.set_multi(mode, stand_in=True, bands=bands)
    for ngpus in (2, 3):
        st = _abi.rg_stats()
        out = np.zeros((36, 64, 4), np.uint8)
        reg = _abi.HostRegistration(out) if pinned else None
        try:
            status = _abi.lib().rg_render_multi(ds.handle, 64, 36, ngpus, 4, out.ctypes.data, C.byref(st))
        finally:
            if reg is not None:
                reg.close()
        assert status == o_st
        assert st.error_pixel == o_err
        assert st.rays.as_dict() == o_counts
        assert np.array_equal(out, o_rgba)
    ds.close()


def test_render_multi_reports_device_errors(oracle_lib):
    scene = _far_sphere_scene(30.0)
    o_st, _, _, _, o_err = _oracle(oracle_lib, scene, 64, 36)
    ds = DeviceScene(scene)
    st = _abi.rg_stats()
    out = np.zeros((36, 64, 4), np.uint8)
    status = _abi.lib().rg_render_multi(ds.handle, 64, 36, 1, 8, out.ctypes.data, C.byref(st))
    ds.close()
    assert status == o_st == _abi.RG_ERR_NAN_DISTANCE
    assert st.error_pixel == o_err
