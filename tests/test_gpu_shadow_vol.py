"""The PLAIN light kernels' shadow mask volume (raingun_amd/csrc/rg_shadow_vol.cpp; the lookup and the
masked walk: rg_render_kernel.h, rg_k_trace.h trace_shadow) on the GPU.

Every frame is rendered twice on one scene handle, with the volume and with it switched off
(rg_debug_set_shadow_volume), as a single and as a pipelined device-resident launch, and compared
byte for byte with the CPU restatement and with each other, with equal ray counts; the debug queries
name the kernel (rg_debug_last_plain) and say whether it ran with the volume
(rg_debug_last_shadow_volume), so no case passes on another path."""
import copy
import math

import numpy as np
import pytest

from gpu_launch import SIZES, assert_same_pixels, device_launch, oracle_frame, require_device
from raingun_amd import _abi
from raingun_amd.color import Color
from raingun_amd.scene import DeviceScene, DirectionalLight, Material, Plane, Scene, Sphere, SphericalLight

pytestmark = pytest.mark.gpu

MODES = ["single", "pipelined"]


@pytest.fixture(scope="module", autouse=True)
def _device():
    require_device()


def _test1(example_scenes, lights=3, depth=5, fov=None):
    s = copy.deepcopy(example_scenes["test1"])
    s.lights = s.lights[:lights]
    s.max_recursion_depth = depth
    if fov is not None:
        s.fov = fov
    return s


def _col(h):
    return Color.from_str(h)


def _floor(y=-2.0):
    return Plane((0.0, y, -5.0), (0.0, -1.0, 0.0), Material(_col("#c8c8b4"), 0.3))


def _mirror_scene():
    """A reflecting sphere beside a diffuse one over a floor: shadow origins from secondary hits."""
    mirror = Material(_col("#ffffff"), 0.5, surface="Reflecting", reflectivity=0.7)
    return Scene(bodies=[_floor(), Sphere((-1.6, -0.5, -6.0), 1.5, mirror), Sphere((1.7, -0.8, -5.5), 1.2, Material(_col("#ff8844"), 0.6))],
                 lights=[DirectionalLight((0.4, -1.0, -0.9), _col("#ffffee"), 5.0),
                         SphericalLight((3.0, 4.0, -2.0), _col("#88aaff"), 3000.0)],
                 default_color=_col("#203040"), max_recursion_depth=5)


def _light_inside_scene():
    return Scene(bodies=[_floor(), Sphere((0.0, 0.5, -7.0), 2.0, Material(_col("#ddddff"), 0.6)),
                         Sphere((3.0, -1.0, -5.0), 1.0, Material(_col("#ffdd88"), 0.6))],
                 lights=[SphericalLight((0.3, 0.8, -6.5), _col("#ffffff"), 4000.0),
                         SphericalLight((-4.0, 5.0, -3.0), _col("#ffeecc"), 5000.0)],
                 default_color=_col("#101820"), max_recursion_depth=3)


def _ulps(x, n):
    for _ in range(abs(n)):
        x = math.nextafter(x, math.inf if n > 0 else -math.inf)
    return x


def _light_on_floor_scene(n):
    """A spherical light n ulps off the floor plane (above for n > 0, inside the ground for n < 0)."""
    return Scene(bodies=[_floor(), Sphere((0.0, -1.0, -6.0), 1.0, Material(_col("#ffffff"), 0.6))],
                 lights=[SphericalLight((1.5, _ulps(-2.0, n), -4.0), _col("#ffffff"), 800.0),
                         SphericalLight((-3.0, 6.0, -3.0), _col("#ffeecc"), 5000.0)],
                 default_color=_col("#101820"), max_recursion_depth=3)


def _ceiling_scene():
    """A ceiling whose normal points along the way to the directional light: the pair (ceiling,
    directional light) is kept in every cell, and a spherical light below it."""
    return Scene(bodies=[_floor(), Plane((0.0, 9.0, 0.0), (0.0, 1.0, 0.0), Material(_col("#8899aa"), 0.5)),
                         Sphere((0.5, -0.5, -6.0), 1.5, Material(_col("#ffccaa"), 0.6))],
                 lights=[DirectionalLight((0.4, -1.0, -0.9), _col("#ffffee"), 5.0),
                         SphericalLight((-3.0, 5.0, -3.0), _col("#ffeecc"), 5000.0)],
                 default_color=_col("#203040"), max_recursion_depth=3)


def _seventeen_spheres():
    mat = Material(_col("#ffcc88"), 0.6)
    return Scene(bodies=[_floor()] + [Sphere((-6.0 + 1.5 * (i % 9), -1.4 + 1.6 * (i // 9), -8.0 - 0.3 * i), 0.6, mat) for i in range(17)],
                 lights=[SphericalLight((-3.0, 6.0, -3.0), _col("#ffeecc"), 5000.0)],
                 default_color=_col("#203040"), max_recursion_depth=3)


def _check(oracle_lib, key, scene, w, h, mode, volume=True, plain=True):
    o_rgba, o_counts = oracle_frame(oracle_lib, key, scene, w, h)
    ds = DeviceScene(scene)
    info = ds.shadow_volume_info()
    assert info["built"] == volume and info["enabled"] == volume
    if volume:
        assert info["g"] ** 3 * 4 == info["bytes"] and 0.0 < info["set_share"] < 1.0
    on = device_launch(ds, w, h, mode)
    ds.set_shadow_volume(False)
    off = device_launch(ds, w, h, mode)
    ds.close()
    if plain is not None:
        assert (on[2], off[2]) == (plain, plain), f"ran the {'PLAIN' if on[2] else 'general'} kernel"
    assert (on[3], off[3]) == (volume, False), "which launch ran with the volume"
    assert on[1] == o_counts and off[1] == o_counts, "ray counts differ"
    assert np.array_equal(on[0], off[0]), "the frame differs from the same launch without the volume"
    assert_same_pixels(on[0], o_rgba, "against the CPU restatement")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("lights", [3, 2, 1])
def test_test1(oracle_lib, example_scenes, lights, w, h, mode):
    """test1 with 3, 2 and 1 of its lights: the LB 3 / 2 / 1 kernels."""
    _check(oracle_lib, ("test1", lights, 5), _test1(example_scenes, lights), w, h, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("share", [0, 7])
def test_eighth_share_against_the_whole_frame(oracle_lib, example_scenes, share, mode):
    """Rows r, r + 8, ... of 8-row tiles (a 1/8 share of rg_render_multi) against the whole frame's rows."""
    w, h = 97, 61
    scene = _test1(example_scenes)
    o_rgba, _ = oracle_frame(oracle_lib, ("test1", 3, 5), scene, w, h)
    ds = DeviceScene(scene)
    on = device_launch(ds, w, h, mode, _abi.rg_tiling(8, 8, share))
    ds.set_shadow_volume(False)
    off = device_launch(ds, w, h, mode, _abi.rg_tiling(8, 8, share))
    ds.close()
    assert (on[2], on[3], off[2], off[3]) == (True, True, True, False)
    assert on[1] == off[1] and on[1]["shadow"] > 0, "ray counts differ"
    assert np.array_equal(on[0], off[0])
    rows = o_rgba[8 * share:min(8 * share + 8, h)]
    assert np.array_equal(on[0][:len(rows)], rows)


@pytest.mark.parametrize("mode", MODES)
def test_depth_16(oracle_lib, example_scenes, mode):
    """9..16 frames: a PLAIN instantiation of rg_render_light_d16.hip."""
    _check(oracle_lib, ("test1", 3, 16), _test1(example_scenes, 3, 16), 64, 40, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h", SIZES)
def test_fov_170(oracle_lib, example_scenes, w, h, mode):
    """Floor hits far outside [-O, O]^3 take the all-ones word, in waves that also hold lanes inside."""
    _check(oracle_lib, ("test1", 3, 5, 170), _test1(example_scenes, fov=170.0), w, h, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ["mirror", "light_inside", "light_above_floor", "light_below_floor", "ceiling"])
def test_scenes(oracle_lib, name, w, h, mode):
    scene = {"mirror": _mirror_scene, "light_inside": _light_inside_scene,
             "light_above_floor": lambda: _light_on_floor_scene(3), "light_below_floor": lambda: _light_on_floor_scene(-3),
             "ceiling": _ceiling_scene}[name]()
    _check(oracle_lib, name, scene, w, h, mode)


@pytest.mark.parametrize("mode", MODES)
def test_seventeen_spheres_have_no_volume(oracle_lib, mode):
    """Past 16 spheres there is no volume: the scene renders as before, whichever kernel it runs."""
    _check(oracle_lib, "seventeen", _seventeen_spheres(), 97, 61, mode, volume=False, plain=None)
