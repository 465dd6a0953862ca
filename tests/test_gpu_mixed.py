"""The mixed-primitive scene family (tests/mixed_scenes.py: spheres, planes, disks and boxes interleaved, all six
materials of each kind) through every kernel family, against the CPU restatement and the references tied to it.

The bar is the project's: RGBA8 byte-identical, pre-quantisation f32 RGB within 1e-4 per channel, the three
ray counts equal, and no PLAIN light kernel for a scene with a disk or a box.  tests/test_mixed_scenes_cpu.py
holds the conditions that keep these tests from passing vacuously (every combination of kind, surface and
coloration that a config can show is the primary hit of some pixels; secondary and shadow rays exist) and pins
the oracle's disk and box arithmetic to the reference's source.  Frames are 97x61 (partial 8x8 tiles) and, for
the first test, 64x40 (whole tiles); every reference is computed once per (config, size) and shared read-only.
"""
import numpy as np
import pytest

import aov_ref
import camera_ref
import lens_ref
import mixed_scenes
import ref_lib
from gpu_launch import SIZES, assert_same_pixels, device_launch, oracle_frame, require_device
from mixed_scenes import CONFIGS, config_scene
from raingun_amd import _abi, aa, aov
from raingun_amd.camera import Camera, Lens
from raingun_amd.scene import DeviceScene, SceneDesc
from test_gpu_parity import PATH_BVH, RGB_TOL

pytestmark = pytest.mark.gpu

W, H = SIZES[0]
PATHS = [_abi.PATH_LIGHT, _abi.PATH_HEAVY]
SIDE = Camera.look_at((8.0, 4.0, -3.0), (0.0, 1.0, -17.0))  # the scene's centre, seen from the right and above
LENS = Lens(0.3, 15.0)


@pytest.fixture(scope="module", autouse=True)
def _device():
    require_device()


def _has_disk_or_box(name):
    c = CONFIGS[name]
    return c.n_dsk + c.n_box > 0 or c.inside


def _oracle(oracle_lib, name, w, h, **tiling):
    """(status, rgba, rgb, counts, error pixel) of the CPU restatement, once per (config, size, tiling)."""
    key = ("mixed", name, w, h, tuple(sorted(tiling.items())))
    return ref_lib.cached(key, oracle_lib.render, SceneDesc(config_scene(name)), w, h, want_rgb=True, **tiling)


def _assert_frame(rgba, rgb, counts, ref, what):
    st, o_rgba, o_rgb, o_counts, err = ref
    assert st == 0 and err == -1, what
    if counts is not None:
        assert counts == o_counts, f"{what}: ray counts differ: {counts} != {o_counts}"
    if rgb is not None:
        diff = float(np.nanmax(np.abs(rgb.astype(np.float64) - o_rgb.astype(np.float64))))
        assert diff <= RGB_TOL, f"{what}: f32 RGB differs by {diff}"
    assert_same_pixels(rgba, o_rgba, what)


def _render_tiles(ds, name, w, h, ref, what):
    st = _abi.rg_stats()
    rgba, rgb = ds.render_tiles(w, h, want_rgb=True, stats=st)
    if _has_disk_or_box(name):
        assert ds.last_plain() is False, f"{what}: a PLAIN light kernel ran on a scene with a disk or a box"
    assert st.error_pixel == -1
    _assert_frame(rgba, rgb, st.rays.as_dict(), ref, what)


# ---------------------------------------------------------------- every config on both paths, with and without the BVH
ROWS = [(name, path, bvh, lane) for name, c in CONFIGS.items() for path, bvh, lane in PATH_BVH
        if not bvh or c.n_sph >= 16]  # RG_BVH_MIN_SPHERES: no BVH is built below 16 spheres


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name,path,bvh,lane", ROWS)
def test_frames(oracle_lib, name, path, bvh, lane, w, h):
    ds = DeviceScene(config_scene(name), path=path, bvh=bvh)
    try:
        if bvh:
            assert ds.bvh_info().built == 1
        if lane is not None:
            ds.set_lane_depth(lane)
        _render_tiles(ds, name, w, h, _oracle(oracle_lib, name, w, h), f"{name} {w}x{h} path {path} bvh {bvh} lane {lane}")
    finally:
        ds.close()


@pytest.mark.parametrize("lightbuf", [True, False])
@pytest.mark.parametrize("name", ["bvh17", "heavy5l", "many"])
def test_light_buffers_beside_disks_and_boxes(oracle_lib, name, lightbuf):
    """The heavy path's BVH walk with the shadow-ray light buffers and the camera buffer serving the spheres
    while disks and boxes are scanned linearly: a shadow ray's only occluder may be one of those."""
    ds = DeviceScene(config_scene(name), path=_abi.PATH_HEAVY, bvh=True)
    try:
        ds.set_lightbuf(lightbuf)
        assert (ds.lightbuf_count() > 0) == lightbuf
        _render_tiles(ds, name, W, H, _oracle(oracle_lib, name, W, H), f"{name} lightbuf {lightbuf}")
    finally:
        ds.close()


# ---------------------------------------------------------------- device-resident launches
@pytest.mark.parametrize("name", ["light3", "bvh17", "heavy32"])
def test_pipelined(oracle_lib, name):
    ds = DeviceScene(config_scene(name))
    try:
        o_rgba, o_counts = oracle_frame(oracle_lib, ("mixed", name), config_scene(name), W, H)
        for rnd in range(2):  # the second launch finds the frame's state in place
            got = device_launch(ds, W, H, mode="pipelined")
            assert got.plain is False
            assert got.counts == o_counts, (name, rnd, got.counts, o_counts)
            assert_same_pixels(got.rgba, o_rgba, f"{name} pipelined launch {rnd}")
    finally:
        ds.close()


@pytest.mark.parametrize("tile_rows,stride,offset", [(8, 3, 1), (7, 2, 0)])
@pytest.mark.parametrize("name", ["light3", "bvh17", "heavy32"])
def test_row_tilings(oracle_lib, name, tile_rows, stride, offset):
    ref = _oracle(oracle_lib, name, W, H, tile_rows=tile_rows, stride=stride, offset=offset)
    ds = DeviceScene(config_scene(name))
    try:
        got = device_launch(ds, W, H, tiling=_abi.rg_tiling(tile_rows, stride, offset))
        assert got.plain is False
        _assert_frame(got.rgba, None, got.counts, ref, f"{name} tiling {tile_rows, stride, offset}")
    finally:
        ds.close()


@pytest.mark.parametrize("name", ["light3", "heavy32", "nosph"])
def test_host_frames(oracle_lib, name):
    """rg_render_image: the host-visible path (the HF heavy kernel, the light kernels' LDS tile ring)."""
    ds = DeviceScene(config_scene(name))
    try:
        st = _abi.rg_stats()
        rgba = ds.render_image(W, H, stats=st)
        assert ds.last_plain() is False and st.error_pixel == -1
        _assert_frame(rgba, None, st.rays.as_dict(), _oracle(oracle_lib, name, W, H), f"{name} render_image")
    finally:
        ds.close()


def test_tile_order(oracle_lib):
    """Probe-ordered tile scheduling, which also keeps a scene off the PLAIN kernels."""
    name = "heavy32"
    ds = DeviceScene(config_scene(name))
    try:
        ds.set_tile_order(1)
        _render_tiles(ds, name, W, H, _oracle(oracle_lib, name, W, H), f"{name} tile order 1")
        got = device_launch(ds, W, H)
        assert got.plain is False
        _assert_frame(got.rgba, None, got.counts, _oracle(oracle_lib, name, W, H), f"{name} tile order 1, device-resident")
    finally:
        ds.close()


# ---------------------------------------------------------------- the camera, lens and sparse families
@pytest.mark.parametrize("name", ["light3", "heavy5l", "inside_box"])
def test_camera(name):
    ref = camera_ref.cached(("mixed", name), config_scene(name), SIDE, W, H)
    assert (ref[1][..., :3] != ref[1][0, 0, :3]).any(), "the pose sees nothing"
    for path in PATHS:
        ds = DeviceScene(config_scene(name), path=path)
        try:
            ds.set_camera(SIDE)
            _render_tiles(ds, name, W, H, ref, f"{name} camera path {path}")
        finally:
            ds.close()


@pytest.mark.parametrize("name", ["light3", "heavy32"])
def test_lens(name):
    w, h, k = SIZES[1][0], SIZES[1][1], 2
    ref = lens_ref.cached(("mixed", name), config_scene(name), None, LENS, w, h, k)
    for path in PATHS:
        ds = DeviceScene(config_scene(name), path=path)
        try:
            ds.set_lens(LENS)
            st = _abi.rg_stats()
            rgba, mean = ds.render_image_aa(w, h, k, want_rgb=True, stats=st)
            assert st.error_pixel == -1
            _assert_frame(rgba, mean, st.rays.as_dict(), ref, f"{name} lens path {path}")
        finally:
            ds.close()


@pytest.mark.parametrize("name", ["light3", "heavy32"])
def test_sparse(oracle_lib, name):
    """rg_render_image_aa_adaptive against raingun_amd.aa.resolve_adaptive over the oracle's 1-sample frame and
    its k W x k H sample frame, as tests/test_gpu_aa_adaptive.py does it."""
    k, t = 2, 32
    _, base_rgba, base_rgb, base_counts, _ = _oracle(oracle_lib, name, W, H)
    _, _, s_rgb, full_counts, _ = _oracle(oracle_lib, name, k * W, k * H)
    want_mean, want_rgba, want_mask = aa.resolve_adaptive(base_rgba, base_rgb, s_rgb, k, t)
    flagged = int(want_mask.sum())
    assert 0 < flagged < W * H, f"the case is vacuous: {flagged} of {W * H} pixels refined"
    for path in PATHS:
        ds = DeviceScene(config_scene(name), path=path)
        try:
            st = _abi.rg_stats()
            rgba, mean, mask = ds.render_image_aa_adaptive(W, H, k, t, want_rgb=True, want_mask=True, stats=st)
            assert np.array_equal(mask, want_mask), f"path {path}: {np.count_nonzero(mask != want_mask)} mask bytes differ"
            assert_same_pixels(rgba, want_rgba, f"{name} sparse path {path}")
            diff = float(np.abs(mean.astype(np.float64) - want_mean.astype(np.float64)).max())
            assert diff <= RGB_TOL, f"path {path}: f32 means differ by {diff}"
            rays = st.rays.as_dict()
            assert rays["primary"] == W * H + k * k * flagged
            for cls in ("shadow", "secondary"):
                assert base_counts[cls] <= rays[cls] <= base_counts[cls] + full_counts[cls], (path, cls)
            assert st.error_pixel == -1
        finally:
            ds.close()


# ---------------------------------------------------------------- the AOV kernel
@pytest.mark.parametrize("name", list(CONFIGS))
def test_aov_layers(name):
    """All five layers bit for bit with the AOV reference: the first GPU check of disk and box `uv` and `albedo`
    (the cross(n, unit_y) fallback of the disks facing down -z, the boxes' constant (0, 0)) and of box normals
    where boxes are common."""
    st_ref, ref, _, err = aov_ref.cached(("mixed", name), config_scene(name), W, H)
    assert st_ref == 0 and err == -1
    ds = DeviceScene(config_scene(name))
    try:
        st = _abi.rg_stats()
        got = ds.render_aov(W, H, stats=st)
        assert st.rays.as_dict() == {"primary": W * H, "shadow": 0, "secondary": 0} and st.error_pixel == -1
        bad = {}
        for n in aov.LAYERS:
            assert got[n].shape == ref[n].shape and got[n].dtype == ref[n].dtype, n
            differ = int((aov_ref.bits(got[n]) != aov_ref.bits(ref[n])).sum())
            print(f"{name} {n}: {differ} values differ")
            if differ:
                bad[n] = differ
        assert not bad, f"{name}: values that differ per layer: {bad}"
    finally:
        ds.close()


# ---------------------------------------------------------------- Scene::trace
@pytest.mark.parametrize("name", ["many", "nosph"])
def test_trace(oracle_lib, name):
    """4096 rays from inside and outside the boxes, one in four with a direction component of exactly 0.0 or
    -0.0 (tests/test_mixed_scenes_cpu.py: the oracle answers them with status 0), and rays onto the very rim of
    the disks that face down -z: body ids equal the oracle's, distances bit for bit where a ray hits."""
    scene = config_scene(name)
    rays, n_rim = mixed_scenes.trace_rays(name)
    st, od, ob = oracle_lib.trace(SceneDesc(scene), rays)
    assert st == 0 and n_rim >= 1
    hit = ob >= 0
    assert 0 < hit.sum() < len(rays)
    for path in PATHS:
        ds = DeviceScene(scene, path=path)
        try:
            gd, gb = ds.trace(rays)
        finally:
            ds.close()
        differ = np.flatnonzero(gb != ob)
        assert differ.size == 0, f"path {path}: {differ.size} body ids differ, first at ray {differ[:4]} of {len(rays)} ({n_rim} rim rays)"
        assert np.array_equal(aov_ref.bits(gd[hit]), aov_ref.bits(od[hit])), f"path {path}: distances differ"
