"""Exact distance ties on the GPU: the scenes of tests/tie_scenes.py (every body twinned; box faces, disks and a
second parametrisation of the plane lying in the floor and in the back wall; touching and concentric spheres; a
light exactly in a plane and one exactly on a sphere) through every route by which a body id reaches closest_add
(raingun_amd/csrc/rg_k_intersect.h) or a shadow ray its decision, against the CPU restatement and the references
tied to it.

Scene::trace keeps the first minimum in YAML order.  The device scans four tables grouped by kind, the sphere
table in BVH leaf order, and rebuilds the rule from ids carried beside the tables (sph_id, pln_id, dsk_id, box_id,
RgSphF2::id in the BVH leaves, the light buffers and the camera buffer); the BVH walk must keep a child whose entry
distance equals the best hit so far.  In seeded-random geometry none of that matters, here most pixels depend on
it: tests/test_tie_scenes_cpu.py holds the counts (>= 5800 of 5917 pixels of every twinned config change when the
body order is reversed, >= 2000 of 4096 rays of every config but `limits` tie).

The bar is the project's: RGBA8 byte-identical, pre-quantisation f32 RGB within RGB_TOL, the three ray counts
equal, rg_trace body ids equal and distances bit for bit.  Frames are 97x61 (partial 8x8 tiles) and 64x40; every
reference is computed once and shared read-only.
"""
import numpy as np
import pytest

import aov_ref
import area_ref
import camera_ref
import lens_ref
import ref_lib
import tie_scenes
from gpu_launch import SIZES, assert_same_pixels, device_launch, oracle_frame, require_device
from raingun_amd import _abi, aa, aov
from raingun_amd.camera import Camera, Lens
from raingun_amd.scene import DeviceScene, SceneDesc, SphericalLight
from test_gpu_parity import PATH_BVH, RGB_TOL
from tie_scenes import CONFIGS, config_scene

pytestmark = pytest.mark.gpu

W, H = SIZES[0]
PATHS = [_abi.PATH_LIGHT, _abi.PATH_HEAVY]
# side-on poses: the twinned mixed scenes' centre from the right and above; the coplanar scenes' floor patch and
# back wall from the right, above the floor and in front of the wall (both planes are one-sided)
POSE = {False: Camera.look_at((8.0, 4.0, -3.0), (0.0, 1.0, -17.0)), True: Camera.look_at((11.0, 2.0, -3.0), (-1.0, -2.0, -18.0))}
LENS = Lens(0.3, 15.0)


@pytest.fixture(scope="module", autouse=True)
def _device():
    require_device()


def _n_sph(name):
    return tie_scenes.counts(name)[0]


def _has_disk_or_box(name):
    return sum(tie_scenes.counts(name)[2:]) > 0


def _pose(name):
    return POSE[CONFIGS[name].coplanar]


def _paths(name):
    return PATHS if len(config_scene(name).lights) <= 3 else [_abi.PATH_HEAVY]  # more lights than a light kernel takes


def _oracle(oracle_lib, name, w, h, **tiling):
    """(status, rgba, rgb, counts, error pixel) of the CPU restatement, once per (config, size, tiling)."""
    key = ("ties", name, w, h, tuple(sorted(tiling.items())))
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
ROWS = [(name, path, bvh, lane) for name in CONFIGS for path, bvh, lane in PATH_BVH
        if not bvh or _n_sph(name) >= 16]  # RG_BVH_MIN_SPHERES: no BVH is built below 16 spheres


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name,path,bvh,lane", ROWS)
def test_frames(oracle_lib, name, path, bvh, lane, w, h):
    ds = DeviceScene(config_scene(name), path=path, bvh=bvh)
    try:
        assert ds.bvh_info().built == (1 if _n_sph(name) >= 16 else 0)
        if bvh:
            assert ds.bvh_info().enabled == 1
        if lane is not None:
            ds.set_lane_depth(lane)
        _render_tiles(ds, name, w, h, _oracle(oracle_lib, name, w, h), f"{name} {w}x{h} path {path} bvh {bvh} lane {lane}")
    finally:
        ds.close()


# ---------------------------------------------------------------- the PLAIN light kernels
@pytest.mark.parametrize("mode", ["single", "pipelined"])
@pytest.mark.parametrize("w,h", SIZES)
def test_plain_kernel_states(oracle_lib, w, h, mode):
    """plain_twins through a PLAIN light kernel with its first-hit tiles on and off and its shadow mask volume on
    and off: each state decides between twins by itself (the first-hit path's own closest hit; the volume's
    masked walk skips bodies, never the winner)."""
    name = "plain_twins"
    o_rgba, o_counts = oracle_frame(oracle_lib, ("ties", name), config_scene(name), w, h)
    voting = tie_scenes.first_hit_tiles(config_scene(name), aov_ref.cached(("ties", name), config_scene(name), w, h)[1]["body"])
    assert 0 < voting.sum() < voting.size  # tests/test_tie_scenes_cpu.py
    ds = DeviceScene(config_scene(name))
    try:
        assert ds.shadow_volume_info()["built"]
        for first_hit in (True, False):
            for volume in (True, False):
                ds.set_first_hit_tiles(first_hit)
                ds.set_shadow_volume(volume)
                got = device_launch(ds, w, h, mode=mode)
                what = f"{name} {w}x{h} {mode} first-hit tiles {first_hit} shadow volume {volume}"
                assert got.plain is True, f"{what}: the general kernel ran"
                assert got.shadow_volume is volume, what
                tiles = ds.last_first_hit_tiles()
                assert tiles == (int(voting.sum()) if first_hit else 0), f"{what}: {tiles} first-hit tiles, {int(voting.sum())} expected"
                assert got.counts == o_counts, f"{what}: ray counts differ: {got.counts} != {o_counts}"
                assert_same_pixels(got.rgba, o_rgba, what)
    finally:
        ds.close()


@pytest.mark.parametrize("name", [n for n in CONFIGS if _has_disk_or_box(n)])
def test_never_plain_beside_disks_and_boxes(oracle_lib, name):
    o_rgba, o_counts = oracle_frame(oracle_lib, ("ties", name), config_scene(name), W, H)
    ds = DeviceScene(config_scene(name), path=_abi.PATH_LIGHT)
    try:
        got = device_launch(ds, W, H)
        assert got.plain is False
        assert got.counts == o_counts
        assert_same_pixels(got.rgba, o_rgba, f"{name} device-resident, light path")
    finally:
        ds.close()


# ---------------------------------------------------------------- the light buffers and the camera buffer
@pytest.mark.parametrize("lightbuf", [True, False])
@pytest.mark.parametrize("name", ["heavy_twins", "heavy5l_twins", "coplanar_bvh"])
def test_light_buffers(oracle_lib, name, lightbuf):
    """The cells hand a leaf test its sphere by table index and the record's RgSphF2::id names it: both twins of
    a pair sit in a cell's list, and coplanar_bvh's fourth light lies exactly on a sphere."""
    ds = DeviceScene(config_scene(name), path=_abi.PATH_HEAVY, bvh=True)
    try:
        ds.set_lightbuf(lightbuf)
        assert (ds.lightbuf_count() > 0) == lightbuf
        if lightbuf:
            assert ds.lightbuf_count() == len(config_scene(name).lights)
        for w, h in SIZES:
            _render_tiles(ds, name, w, h, _oracle(oracle_lib, name, w, h), f"{name} {w}x{h} lightbuf {lightbuf}")
    finally:
        ds.close()


# ---------------------------------------------------------------- the other launches
LAUNCHED = ["light_twins", "heavy_twins", "coplanar", "coplanar_bvh"]  # auto: light, heavy + BVH, light, heavy + BVH


@pytest.mark.parametrize("name", LAUNCHED)
def test_pipelined(oracle_lib, name):
    ds = DeviceScene(config_scene(name))
    try:
        o_rgba, o_counts = oracle_frame(oracle_lib, ("ties", name), config_scene(name), W, H)
        for rnd in range(2):  # the second launch finds the frame's state in place
            got = device_launch(ds, W, H, mode="pipelined")
            assert got.plain is False
            assert got.counts == o_counts, (name, rnd, got.counts, o_counts)
            assert_same_pixels(got.rgba, o_rgba, f"{name} pipelined launch {rnd}")
    finally:
        ds.close()


@pytest.mark.parametrize("name", LAUNCHED)
def test_row_tiling(oracle_lib, name):
    tile_rows, stride, offset = 8, 3, 1
    ref = _oracle(oracle_lib, name, W, H, tile_rows=tile_rows, stride=stride, offset=offset)
    ds = DeviceScene(config_scene(name))
    try:
        got = device_launch(ds, W, H, tiling=_abi.rg_tiling(tile_rows, stride, offset))
        _assert_frame(got.rgba, None, got.counts, ref, f"{name} tiling {tile_rows, stride, offset}")
    finally:
        ds.close()


@pytest.mark.parametrize("name", LAUNCHED + ["plain_twins"])
def test_host_frames(oracle_lib, name):
    """rg_render_image: the host-visible path (the HF heavy kernel, the light kernels' LDS tile ring)."""
    ds = DeviceScene(config_scene(name))
    try:
        st = _abi.rg_stats()
        rgba = ds.render_image(W, H, stats=st)
        assert st.error_pixel == -1
        _assert_frame(rgba, None, st.rays.as_dict(), _oracle(oracle_lib, name, W, H), f"{name} render_image")
    finally:
        ds.close()


@pytest.mark.parametrize("name", LAUNCHED)
def test_tile_order(oracle_lib, name):
    ds = DeviceScene(config_scene(name))
    try:
        ds.set_tile_order(1)
        _render_tiles(ds, name, W, H, _oracle(oracle_lib, name, W, H), f"{name} tile order 1")
        got = device_launch(ds, W, H)
        assert got.plain is False
        _assert_frame(got.rgba, None, got.counts, _oracle(oracle_lib, name, W, H), f"{name} tile order 1, device-resident")
    finally:
        ds.close()


# ---------------------------------------------------------------- the camera, lens, area and sparse families
@pytest.mark.parametrize("name", ["heavy_twins", "light_twins", "coplanar", "coplanar_bvh"])
def test_camera(name):
    ref = camera_ref.cached(("ties", name), config_scene(name), _pose(name), W, H)
    assert len(np.unique(ref[1].reshape(-1, 4), axis=0)) >= 100, "the pose sees next to nothing"
    for path in _paths(name):
        ds = DeviceScene(config_scene(name), path=path)
        try:
            ds.set_camera(_pose(name))
            _render_tiles(ds, name, W, H, ref, f"{name} camera path {path}")
        finally:
            ds.close()


@pytest.mark.parametrize("name", ["heavy_twins", "bvh16_twins", "coplanar", "coplanar_bvh"])
def test_lens(name):
    """Every sample has its own origin on the lens: the BVH walk's far-origin shift and the slab tests start
    somewhere else for each, and the twins still tie to the bit."""
    w, h, k = SIZES[1][0], SIZES[1][1], 2
    ref = lens_ref.cached(("ties", name), config_scene(name), _pose(name), LENS, w, h, k)
    for path in _paths(name):
        ds = DeviceScene(config_scene(name), path=path)
        try:
            ds.set_camera(_pose(name))
            ds.set_lens(LENS)
            st = _abi.rg_stats()
            rgba, mean = ds.render_image_aa(w, h, k, want_rgb=True, stats=st)
            assert st.error_pixel == -1
            _assert_frame(rgba, mean, st.rays.as_dict(), ref, f"{name} lens path {path}")
        finally:
            ds.close()


def _radii(scene):
    return tuple(0.25 + 0.125 * i if isinstance(l, SphericalLight) else 0.0 for i, l in enumerate(scene.lights))


@pytest.mark.parametrize("name", ["heavy_twins", "bvh16_twins", "coplanar", "coplanar_bvh"])
def test_area(name):
    """Area lights (every spherical light a radius > 0) through the lens: a shadow ray per sample towards its own
    point of the light, past twins and across the coplanar patches."""
    w, h, k = SIZES[1][0], SIZES[1][1], 2
    scene = config_scene(name)
    radii = _radii(scene)
    assert sum(r > 0.0 for r in radii) >= 2
    ref = area_ref.cached(("ties", name), scene, _pose(name), LENS, radii, w, h, k)
    for path in _paths(name):
        ds = DeviceScene(scene, path=path)
        try:
            ds.set_camera(_pose(name))
            ds.set_lens(LENS)
            ds.set_light_radii(radii)
            st = _abi.rg_stats()
            rgba, mean = ds.render_image_aa(w, h, k, want_rgb=True, stats=st)
            assert st.error_pixel == -1
            _assert_frame(rgba, mean, st.rays.as_dict(), ref, f"{name} area path {path}")
        finally:
            ds.close()


@pytest.mark.parametrize("name", ["heavy_twins", "light_twins", "coplanar", "coplanar_bvh"])
def test_sparse(oracle_lib, name):
    """rg_render_image_aa_adaptive against raingun_amd.aa.resolve_adaptive over the oracle's 1-sample frame and
    its k W x k H sample frame, as tests/test_gpu_mixed.py does it."""
    k, t = 2, 32
    _, base_rgba, base_rgb, base_counts, _ = _oracle(oracle_lib, name, W, H)
    _, _, s_rgb, full_counts, _ = _oracle(oracle_lib, name, k * W, k * H)
    want_mean, want_rgba, want_mask = aa.resolve_adaptive(base_rgba, base_rgb, s_rgb, k, t)
    flagged = int(want_mask.sum())
    assert 0 < flagged < W * H, f"the case is vacuous: {flagged} of {W * H} pixels refined"
    for path in _paths(name):
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
@pytest.mark.parametrize("pose", [False, True])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_aov_layers(name, pose):
    """All five layers bit for bit: a wrong winner stands in the `body` layer itself, and in `uv` and `albedo`
    where a textured body has a textured twin."""
    cam = _pose(name) if pose else None
    st_ref, ref, _, err = aov_ref.cached(("ties", name), config_scene(name), W, H, cam)
    assert st_ref == 0 and err == -1
    ds = DeviceScene(config_scene(name))
    try:
        ds.set_camera(cam)
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
TRACED = ["light_twins", "bvh16_twins", "heavy_twins", "coplanar", "coplanar_bvh"]


@pytest.mark.parametrize("name,path,bvh,lane", [r for r in ROWS if r[0] in TRACED])
def test_trace(oracle_lib, name, path, bvh, lane):
    """tie_scenes.trace_rays: 4096 rays from the origin, from inside the scene and from 100 and 2000 units out,
    most of them with two or more bodies at the bit-equal minimum: body ids equal the oracle's, distances bit for
    bit where a ray hits."""
    scene, rays = config_scene(name), tie_scenes.trace_rays(name)
    st, od, ob = ref_lib.cached(("ties trace", name), oracle_lib.trace, SceneDesc(scene), rays)
    assert st == 0
    hit = ob >= 0
    assert hit.sum() > len(rays) // 2
    ds = DeviceScene(scene, path=path, bvh=bvh)
    try:
        if lane is not None:
            ds.set_lane_depth(lane)
        gd, gb = ds.trace(rays)
    finally:
        ds.close()
    differ = np.flatnonzero(gb != ob)
    assert differ.size == 0, (f"path {path} bvh {bvh} lane {lane}: {differ.size} body ids differ, first at rays {differ[:4]}: "
                              f"{gb[differ[:4]]} for {ob[differ[:4]]}")
    assert np.array_equal(aov_ref.bits(gd[hit]), aov_ref.bits(od[hit])), f"path {path} bvh {bvh}: distances differ"
