"""The PLAIN light kernels' first-hit path (raingun_amd/csrc/rg_render_kernel.h) on the GPU.

Every frame is rendered twice on one scene handle, with the path and with it switched off
(rg_debug_set_first_hit_tiles), as a single and as a pipelined device-resident launch, and compared byte for
byte with the CPU restatement and with each other, with equal ray counts.  rg_debug_last_plain names the
kernel, and rg_debug_last_first_hit_tiles says how many tiles finished on the path: 0 when it is off, and
otherwise exactly the tiles that pass the vote, counted here from the reference's per-pixel primary body
ids (tests/aov_ref.py) -- so no case passes on the other path, and the vote's edge tiles are pinned."""
import copy

import numpy as np
import pytest

import aov_ref
from gpu_launch import SIZES, assert_same_pixels, device_launch, oracle_frame, require_device
from raingun_amd import _abi
from raingun_amd.color import Color
from raingun_amd.scene import DeviceScene, DirectionalLight, Material, Plane, Scene, Sphere, SphericalLight, Texture

pytestmark = pytest.mark.gpu

MODES = ["single", "pipelined"]


@pytest.fixture(scope="module", autouse=True)
def _device():
    require_device()


def _test1(example_scenes, lights=3, depth=5):
    s = copy.deepcopy(example_scenes["test1"])
    s.lights = s.lights[:lights]
    s.max_recursion_depth = depth
    return s


def _col(h):
    return Color.from_str(h)


def _floor(y=-2.0):
    return Plane((0.0, y, -5.0), (0.0, -1.0, 0.0), Material(_col("#c8c8b4"), 0.3))


def _mirror_scene():
    """tests/test_gpu_shadow_vol.py's: a reflecting sphere beside a diffuse one over a floor."""
    mirror = Material(_col("#ffffff"), 0.5, surface="Reflecting", reflectivity=0.7)
    return Scene(bodies=[_floor(), Sphere((-1.6, -0.5, -6.0), 1.5, mirror), Sphere((1.7, -0.8, -5.5), 1.2, Material(_col("#ff8844"), 0.6))],
                 lights=[DirectionalLight((0.4, -1.0, -0.9), _col("#ffffee"), 5.0),
                         SphericalLight((3.0, 4.0, -2.0), _col("#88aaff"), 3000.0)],
                 default_color=_col("#203040"), max_recursion_depth=5)


def _light_inside_scene():
    """tests/test_gpu_shadow_vol.py's: a spherical light inside a diffuse sphere."""
    return Scene(bodies=[_floor(), Sphere((0.0, 0.5, -7.0), 2.0, Material(_col("#ddddff"), 0.6)),
                         Sphere((3.0, -1.0, -5.0), 1.0, Material(_col("#ffdd88"), 0.6))],
                 lights=[SphericalLight((0.3, 0.8, -6.5), _col("#ffffff"), 4000.0),
                         SphericalLight((-4.0, 5.0, -3.0), _col("#ffeecc"), 5000.0)],
                 default_color=_col("#101820"), max_recursion_depth=3)


def _seventeen_spheres():
    """tests/test_gpu_shadow_vol.py's: past 16 spheres a scene has no shadow mask volume."""
    mat = Material(_col("#ffcc88"), 0.6)
    return Scene(bodies=[_floor()] + [Sphere((-6.0 + 1.5 * (i % 9), -1.4 + 1.6 * (i // 9), -8.0 - 0.3 * i), 0.6, mat) for i in range(17)],
                 lights=[SphericalLight((-3.0, 6.0, -3.0), _col("#ffeecc"), 5000.0)],
                 default_color=_col("#203040"), max_recursion_depth=3)


def _checker(w, h):
    """A w x h RGBA texture (neither a power of two) with a different colour in every texel."""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(40 + 29 * x + 7 * y) % 256, (200 - 17 * x + 31 * y) % 256, (90 + 53 * ((x + y) % 2) + 11 * y) % 256,
                     np.full((h, w), 255)], axis=2).astype(np.uint8)


def _all_diffuse_scene():
    """A textured plane, a textured sphere and a coloured sphere under a directional and a spherical light.
    The floor lies below the eye, so the frame's upper rows see the sky."""
    floor = Plane((0.0, -2.0, -5.0), (0.0, -1.0, 0.0), Material(Texture("floor", _checker(7, 5), 0.25, 0.5), 0.4))
    ball = Sphere((-1.2, -0.6, -5.0), 1.4, Material(Texture("ball", _checker(6, 9), 0.0, 0.125), 0.6))
    return Scene(bodies=[floor, ball, Sphere((1.8, -1.0, -6.0), 1.0, Material(_col("#66cc88"), 0.7))],
                 lights=[DirectionalLight((0.4, -1.0, -0.9), _col("#ffffee"), 4.0),
                         SphericalLight((2.0, 4.0, -3.0), _col("#ffddaa"), 2500.0)],
                 default_color=_col("#4070a0"), max_recursion_depth=5)


FAR = 9e99


def _far_plane_scene():
    """A diffuse wall at z = -9e99 behind a near sphere, fov 120: every parameter is below 1e100, so the scene
    is no NaN scene and runs PLAIN, but the wall's hit points d * t leave [-1e100, 1e100]^3 wherever
    |d.x / d.z| or |d.y / d.z| exceeds 10 / 9 -- their shadow batches are ray_exotic."""
    return Scene(bodies=[Plane((0.0, 0.0, -FAR), (0.0, 0.0, -1.0), Material(_col("#c0b0a0"), 0.5)),
                         Sphere((0.0, 0.0, -6.0), 1.0, Material(_col("#ff8844"), 0.6))],
                 lights=[DirectionalLight((0.3, -0.2, -1.0), _col("#ffffff"), 3.0)],
                 default_color=_col("#203040"), max_recursion_depth=3, fov=120.0)


def _simple_pixels(geom_key, scene, w, h):
    """(H, W) bool: the pixel's primary ray ends at a miss, a Diffuse body, or a Reflecting body at the depth limit."""
    st, layers, _, _ = aov_ref.cached(geom_key, scene, w, h)
    assert st == 0
    ok = np.array([b.material.surface == "Diffuse" or (b.material.surface == "Reflecting" and scene.max_recursion_depth <= 1)
                   for b in scene.bodies] + [True])  # [-1]: a miss
    return ok[layers["body"]], layers


def _tile_all(px):
    """(tile rows, tile columns) bool: every pixel of the 8x8 tile inside the frame is set."""
    h, w = px.shape
    pad = np.ones(((h + 7) // 8 * 8, (w + 7) // 8 * 8), dtype=bool)
    pad[:h, :w] = px
    return pad.reshape(pad.shape[0] // 8, 8, pad.shape[1] // 8, 8).all(axis=(1, 3))


def _check(oracle_lib, key, scene, w, h, mode, geom_key=None, voting=None, bvh=None):
    """-> (the frame, the voting tiles): the checks every case makes, for the tiles `voting` or the vote's own."""
    o_rgba, o_counts = oracle_frame(oracle_lib, key, scene, w, h)
    if voting is None:
        voting = _tile_all(_simple_pixels(geom_key or key, scene, w, h)[0])
    ds = DeviceScene(scene, bvh=bvh)
    on = device_launch(ds, w, h, mode)
    n_on = ds.last_first_hit_tiles()
    ds.set_first_hit_tiles(False)
    off = device_launch(ds, w, h, mode)
    n_off = ds.last_first_hit_tiles()
    ds.close()
    assert (on.plain, off.plain) == (True, True), "ran the general kernel"
    assert on.counts == o_counts and off.counts == o_counts, "ray counts differ"
    assert np.array_equal(on.rgba, off.rgba), "the frame differs from the same launch without the path"
    assert_same_pixels(on.rgba, o_rgba, "against the CPU restatement")
    assert n_off == 0, "tiles on the path while it is switched off"
    assert n_on == int(voting.sum()), f"{n_on} tiles on the path, {int(voting.sum())} of {voting.size} pass the vote"
    return on.rgba, voting


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("lights", [3, 2, 1])
def test_test1(oracle_lib, example_scenes, lights, w, h, mode):
    """test1 with 3, 2 and 1 of its lights: the LB 3 / 2 / 1 kernels, both paths in one frame."""
    _, voting = _check(oracle_lib, ("test1", lights, 5), _test1(example_scenes, lights), w, h, mode, geom_key="test1")
    assert (int(voting.sum()), voting.size) == {(97, 61): (83, 104), (64, 40): (30, 40)}[(w, h)]  # tests/test_first_hit_tiles_cpu.py


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [16, 40])
def test_deep_stacks(oracle_lib, example_scenes, depth, mode):
    """9..16 and 17..64 frames: the PLAIN instantiations of rg_render_light_d16.hip and _d64.hip."""
    _check(oracle_lib, ("test1", 3, depth), _test1(example_scenes, 3, depth), 64, 40, mode, geom_key="test1")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h", SIZES)
def test_depth_1(oracle_lib, example_scenes, w, h, mode):
    """max_depth 1: the reflecting sphere's hits mix with the default colour on the path (kind 1); only
    the tiles that see the refractive sphere stay outside."""
    scene = _test1(example_scenes, 3, 1)
    _, voting = _check(oracle_lib, ("test1", 3, 1), scene, w, h, mode, geom_key="test1")
    _, layers = _simple_pixels("test1", scene, w, h)
    surfaces = [b.material.surface for b in scene.bodies]
    assert sorted(set(surfaces)) == ["Diffuse", "Reflecting", "Refractive"] and surfaces.count("Refractive") == 1
    assert np.isin(layers["body"], [i for i, s in enumerate(surfaces) if s == "Reflecting"]).any()
    assert np.array_equal(voting, _tile_all(layers["body"] != surfaces.index("Refractive")))
    assert 0 < voting.sum() < voting.size


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h", SIZES)
def test_all_diffuse(oracle_lib, w, h, mode):
    """Every tile takes the path: textured and coloured hits, partial tiles, and whole tiles of sky, which
    store the default colour."""
    scene = _all_diffuse_scene()
    rgba, voting = _check(oracle_lib, "fh_all_diffuse", scene, w, h, mode)
    assert voting.all()
    st, layers, _, _ = aov_ref.cached("fh_all_diffuse", scene, w, h)
    sky = _tile_all(layers["body"] < 0)
    assert sky.sum() >= w // 8 and not sky.all(), "whole tiles of sky, and tiles with hits"
    sky_px = np.repeat(np.repeat(sky, 8, axis=0), 8, axis=1)[:h, :w]
    d = scene.default_color
    want = [int(np.float32(c) * np.float32(255.0)) for c in (d.red, d.green, d.blue)] + [255]
    assert (rgba[sky_px] == np.array(want, dtype=np.uint8)).all()
    assert {b for b in np.unique(layers["body"])} == {-1, 0, 1, 2}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ["mirror", "light_inside"])
def test_scenes(oracle_lib, name, w, h, mode):
    """A reflecting sphere (its tiles go the general way, their secondary hits' batches too) and a light inside a sphere."""
    scene = {"mirror": _mirror_scene, "light_inside": _light_inside_scene}[name]()
    _, voting = _check(oracle_lib, name, scene, w, h, mode)
    assert voting.all() == (name == "light_inside")


@pytest.mark.parametrize("mode", MODES)
def test_seventeen_spheres(oracle_lib, mode):
    """Past 16 spheres there is no volume: every word is all ones and the walk tests every body.  (From 16
    spheres on a scene has a BVH and light buffers, which the PLAIN kernels do not take: switched off here.)"""
    scene = _seventeen_spheres()
    ds = DeviceScene(scene)
    assert not ds.shadow_volume_info()["built"]
    ds.close()
    _, voting = _check(oracle_lib, "seventeen", scene, 97, 61, mode, bvh=False)
    assert voting.all()


@pytest.mark.parametrize("mode", MODES)
def test_eighth_share_against_the_whole_frame(oracle_lib, example_scenes, mode):
    """Rows 56..60 of 8-row tiles (the last 1/8 share of rg_render_multi, a partial tile row) against the whole frame's."""
    w, h, share = 97, 61, 7
    scene = _test1(example_scenes)
    o_rgba, _ = oracle_frame(oracle_lib, ("test1", 3, 5), scene, w, h)
    voting = _tile_all(_simple_pixels("test1", scene, w, h)[0])[share]
    ds = DeviceScene(scene)
    on = device_launch(ds, w, h, mode, _abi.rg_tiling(8, 8, share))
    n_on = ds.last_first_hit_tiles()
    ds.set_first_hit_tiles(False)
    off = device_launch(ds, w, h, mode, _abi.rg_tiling(8, 8, share))
    n_off = ds.last_first_hit_tiles()
    ds.close()
    assert (on.plain, off.plain) == (True, True)
    assert on.counts == off.counts and on.counts["shadow"] > 0, "ray counts differ"
    assert np.array_equal(on.rgba, off.rgba)
    rows = o_rgba[8 * share:min(8 * share + 8, h)]
    assert len(rows) == 5 and np.array_equal(on.rgba[:len(rows)], rows)
    assert n_off == 0 and n_on == int(voting.sum()) and 0 < n_on


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h", SIZES)
def test_exotic_batches_bail(oracle_lib, w, h, mode):
    """A tile with a hit whose shadow origin leaves [-1e100, 1e100]^3 passes the vote and then bails: it goes
    the general way, whose exact queries the CPU restatement mirrors, and is not counted.  The tiles around
    the near sphere, and the wall's within the bound, stay on the path."""
    scene = _far_plane_scene()
    simple, layers = _simple_pixels("fh_far_plane", scene, w, h)
    assert simple.all()
    # the hit point as the kernel forms it: 0 + d * t, with the reference's own d and t; the wall's normal
    # has no x and no y, so the shadow origin h + n * 1e-13 keeps the hit's x and y, and its z is -9e99
    d = aov_ref.prime_rays(scene.fov, w, h, np.tan(np.radians(np.float64(scene.fov)) / 2.0)).reshape(h, w, 6)[..., 3:]
    hp = d * layers["depth"][..., None]
    exotic = (layers["body"] == 0) & ~(np.abs(hp) < 1e100).all(axis=2)
    margin = np.abs(np.abs(hp[layers["body"] == 0]) / 1e100 - 1.0).min()
    assert margin > 1e-9, "a hit within rounding of the bound: the prediction would depend on tan's last bit"
    voting = _tile_all(~exotic)
    assert 0 < voting.sum() < voting.size and (layers["body"] == 1).any()
    _check(oracle_lib, "fh_far_plane", scene, w, h, mode, voting=voting)
