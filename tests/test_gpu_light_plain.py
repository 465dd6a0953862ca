"""The PLAIN specialisation of the light kernels (rg_render_kernel.h; selection: rg_render_launch.h
rg_light_plain) against the CPU restatement, written like _compare of tests/test_gpu_parity.py.

Device-resident launches only (rg_render_tiles_async / rg_render_tiles_pipelined into device
buffers): RGBA8 byte for byte, per-class ray counts equal, and the debug query
(rg_debug_last_plain) names the kernel every case ran, so none passes on the other path.
"single" launches run the persistent-wave instantiations (TPW -1), "pipelined" ones the
tiles-per-wave grid (TPW 0).  Scenes that miss exactly one PLAIN condition must take the old kernel.
"""
import copy

import numpy as np
import pytest

from gpu_launch import SIZES, assert_same_pixels, device_launch, oracle_frame, require_device
from raingun_amd.color import Color
from raingun_amd.scene import DeviceScene, DirectionalLight, Disk, Material, Scene, Sphere, SphericalLight

pytestmark = pytest.mark.gpu

DEPTHS = [0, 1, 5]


@pytest.fixture(scope="module", autouse=True)
def _device():
    require_device()


def _test1(example_scenes, lights=3, depth=5):
    s = copy.deepcopy(example_scenes["test1"])
    s.lights = s.lights[:lights]
    s.max_recursion_depth = depth
    return s


def _pair_scene():
    """A refractive sphere inside a reflecting one that also encloses the camera: every path
    alternates refraction frames and reflection frames until the depth limit."""
    glass = Material(Color.from_str("#f0fff0"), 0.2, surface="Refractive", index=1.5, transparency=0.9)
    mirror = Material(Color.from_str("#ffd0a0"), 0.6, surface="Reflecting", reflectivity=0.6)
    return Scene(bodies=[Sphere((0.0, 0.0, -5.0), 12.0, mirror), Sphere((0.5, -0.3, -4.0), 1.5, glass)],
                 lights=[SphericalLight((2.0, 3.0, -3.0), Color.from_str("#ffffee"), 900.0),
                         DirectionalLight((0.3, -1.0, -0.4), Color.from_str("#ffffff"), 2.0)],
                 default_color=Color.from_str("#203040"), max_recursion_depth=5)


def _check(oracle_lib, key, scene, w, h, mode, expect_plain, want_rgb=False, prepare=None):
    o_rgba, o_counts = oracle_frame(oracle_lib, key, scene, w, h)
    ds = DeviceScene(scene)
    if prepare:
        prepare(ds)
    rgba, counts, plain, _ = device_launch(ds, w, h, mode, want_rgb=want_rgb)
    ds.close()
    assert plain == expect_plain, f"ran the {'PLAIN' if plain else 'general'} kernel"
    assert counts == o_counts, "ray counts differ"
    assert_same_pixels(rgba, o_rgba)


@pytest.mark.parametrize("mode", ["single", "pipelined"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("lights", [3, 2, 1])
def test_plain_test1(oracle_lib, example_scenes, lights, w, h, depth, mode):
    """test1 as shipped (3 lights, LB 3), cut to 2 lights (LB 2) and to one (the one-light batch)."""
    _check(oracle_lib, ("test1", lights, depth), _test1(example_scenes, lights, depth), w, h, mode, True)


@pytest.mark.parametrize("mode", ["single", "pipelined"])
@pytest.mark.parametrize("w,h", SIZES)
def test_plain_refractive_inside_reflective(oracle_lib, w, h, mode):
    _check(oracle_lib, "pair", _pair_scene(), w, h, mode, True)


@pytest.mark.parametrize("mode", ["single", "pipelined"])
@pytest.mark.parametrize("depth", [12, 20])
def test_plain_deeper_frame_arrays(oracle_lib, example_scenes, depth, mode):
    """9..16 and 17..64 frames: the PLAIN instantiations of rg_render_light_d16.hip / _d64.hip."""
    _check(oracle_lib, ("test1", 3, depth), _test1(example_scenes, 3, depth), 64, 40, mode, True)


def _plus_disk(example_scenes, depth):
    s = _test1(example_scenes, 3, depth)
    s.bodies.append(Disk((1.5, -0.5, -4.0), (0.2, -0.5, -1.0), 0.8, Material(Color.from_str("#ffcc88"), 0.5)))
    return s


def _nan_scene(example_scenes, depth):
    s = _test1(example_scenes, 3, depth)
    s.bodies.append(Sphere((1e100, 0.0, -5.0), 1.0, Material(Color.from_str("#ffffff"), 0.5)))
    return s


# (name, scene builder, f32 RGB requested, scene-handle setting): each misses exactly one PLAIN condition
GENERAL = {
    "disk": (_plus_disk, False, None),
    "aabb": (lambda ex, depth: _with_depth(ex["test3"], depth), False, None),
    "rgb": (lambda ex, depth: _test1(ex, 3, depth), True, None),
    "tile_order": (lambda ex, depth: _test1(ex, 3, depth), False, lambda ds: ds.set_tile_order(1)),
    "nan_scene": (_nan_scene, False, None),
}


def _with_depth(scene, depth):
    s = copy.deepcopy(scene)
    s.max_recursion_depth = depth
    return s


@pytest.mark.parametrize("mode", ["single", "pipelined"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", sorted(GENERAL))
def test_one_condition_missing_takes_the_general_kernel(oracle_lib, example_scenes, name, w, h, depth, mode):
    build, want_rgb, prepare = GENERAL[name]
    scene = build(example_scenes, depth)
    key = ("test1", 3, depth) if name in ("rgb", "tile_order") else (name, depth)
    _check(oracle_lib, key, scene, w, h, mode, False, want_rgb=want_rgb, prepare=prepare)


def test_switching_kernels_on_one_stream_and_handle(oracle_lib, example_scenes):
    """PLAIN, general (f32 RGB requested), PLAIN again on the same stream and scene handle: the
    launch context's two counter sets (each kernel zeroes the other one for the next launch) survive
    the change of kernel -- frames byte-equal to the first ones, ray counts exact every time."""
    import torch

    w, h = 97, 61
    scene = _test1(example_scenes, 3, 5)
    o_rgba, o_counts = oracle_frame(oracle_lib, ("test1", 3, 5), scene, w, h)
    ds = DeviceScene(scene)
    stream = torch.cuda.Stream()
    first = {}
    for want_rgb in (False, True, False, True, False):
        rgba, counts, plain, _ = device_launch(ds, w, h, "single", want_rgb=want_rgb, stream=stream)
        assert plain == (not want_rgb)
        assert counts == o_counts
        assert np.array_equal(rgba, first.setdefault(want_rgb, rgba))
        assert np.array_equal(rgba, o_rgba)
    ds.release_stream(stream.cuda_stream)
    ds.close()
