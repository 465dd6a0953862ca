"""The PLAIN light kernels without the reference's divisions by launch constants (DESIGN.md 4r;
raingun_amd/csrc/rg_exact.h): the camera ray from host reciprocals and unscaled sqrt / reciprocal,
the texture wrap from the dimensions' magics, the planes' texture axes from the host's table, the
tile start from the magic of tiles per row.  Everything must stay bit for bit:

  * rg_debug_camera_check computes every pixel's camera direction both ways on the device: no pixel differs;
  * frames of textured scenes -- a plane on the fallback axis, an oblique one, spheres, offsets
    below zero and above one, negative texture coordinates, each golden texture -- equal the CPU
    restatement byte for byte, with equal ray counts, as a single and as a pipelined launch, and
    rg_debug_last_plain says the PLAIN kernel ran;
  * 1/N shares (a row mapping that is not the identity; tile rows that are and are not a power of
    two) equal the same rows of the whole frame;
  * with the quotient check switched off the launch takes the general kernel and stays exact.
"""
import copy

import numpy as np
import pytest

import gpu_launch
from gpu_launch import SIZES, assert_same_pixels, device_launch, oracle_frame, require_device
from raingun_amd import _abi
from raingun_amd.color import Color
from raingun_amd.scene import (DeviceScene, DirectionalLight, Material, Plane, Scene, Sphere,
                               SphericalLight, Texture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    require_device()


# ---------------------------------------------------------------- the camera ray, both ways
@pytest.fixture(scope="module")
def any_scene():
    ds = DeviceScene(gpu_launch.any_scene())
    yield ds
    ds.close()


@pytest.mark.parametrize("fov", [1.0, 60.0, 90.0, 179.0])
@pytest.mark.parametrize("w,h", [(97, 61), (64, 40), (4096, 8), (1, 1)])
def test_camera_directions_are_bitwise_equal(any_scene, w, h, fov):
    bad, admitted = any_scene.camera_check(w, h, fov)
    print(f"{w}x{h} fov {fov}: {bad} of {w * h} camera directions differ; admitted {admitted}")
    assert admitted, "the launcher's checks refuse this frame"
    assert bad == 0


# ---------------------------------------------------------------- textured frames
def _golden_images(example_scenes):
    """{path: (h, w, 4) uint8} of the golden textures, as the example scenes loaded them."""
    out = {}
    for name in ("test1", "test3"):
        for b in example_scenes[name].bodies:
            c = b.material.coloration
            if isinstance(c, Texture):
                out[c.path] = c.image
    return out


def _tex(images, key, xoff=0.0, yoff=0.0):
    (name,) = [k for k in images if key in k]
    return Texture(name, images[name], xoff, yoff)


LIGHTS = [SphericalLight((2.0, 3.0, -2.0), Color.from_str("#ffffee"), 700.0),
          DirectionalLight((0.3, -1.0, -0.4), Color.from_str("#ffffff"), 1.5)]
MIRROR = Material(Color.from_str("#ffd0a0"), 0.6, surface="Reflecting", reflectivity=0.5)


def _scenes(example_scenes):
    im = _golden_images(example_scenes)
    assert len(im) == 3, sorted(im)
    glass = Material(_tex(im, "land", 0.25, -1.5), 0.3, surface="Refractive", index=1.4, transparency=0.8)
    return {
        # a wall facing the camera: its normal lies along z, so x = n x (0,0,1) vanishes and the
        # fallback axis n x (0,1,0) is taken; clay is 1500 x 1500 (no power of two)
        "wall_z": Scene(bodies=[Plane((0.0, 0.0, -9.0), (0.0, 0.0, -1.0), Material(_tex(im, "clay"), 0.5)),
                                Sphere((0.4, -0.2, -5.0), 1.2, MIRROR)], lights=LIGHTS, max_recursion_depth=5),
        # an oblique plane, offsets below zero and above one; tile1 is 512 x 512
        "oblique": Scene(bodies=[Plane((0.0, -2.0, -5.0), (0.36, -0.48, -0.8), Material(_tex(im, "tile1", -0.75, 2.5), 0.5)),
                                 Sphere((-0.5, 0.3, -4.0), 0.9, MIRROR)], lights=LIGHTS, max_recursion_depth=5),
        # textured spheres, diffuse and refractive (land is 2048 x 1024), over a reflecting textured floor
        "spheres": Scene(bodies=[Plane((0.0, -2.0, 0.0), (0.0, -1.0, 0.0),
                                       Material(_tex(im, "clay", 1.5, -0.5), 0.4, surface="Reflecting", reflectivity=0.3)),
                                 Sphere((-1.2, 0.0, -4.5), 1.3, Material(_tex(im, "land"), 0.6)),
                                 Sphere((1.3, -0.4, -3.5), 1.0, glass)], lights=LIGHTS, max_recursion_depth=5),
        # a floor whose origin lies far to the right of and behind the camera: every hit's texture
        # coordinates are negative on both axes (the wrap's `+ max` branch), one light
        "negative": Scene(bodies=[Plane((60.0, -2.0, 40.0), (0.0, -1.0, 0.0), Material(_tex(im, "tile1", -0.3, -0.7), 0.5)),
                                  Sphere((0.0, -0.5, -5.0), 1.0, MIRROR)], lights=LIGHTS[:1], max_recursion_depth=5),
    }


def _check_frame(oracle_lib, key, scene, w, h, mode, expect_plain=True, prepare=None):
    o_rgba, o_counts = oracle_frame(oracle_lib, key, scene, w, h)
    ds = DeviceScene(scene)
    if prepare:
        prepare(ds)
    rgba, counts, plain, _ = device_launch(ds, w, h, mode)
    ds.close()
    assert plain == expect_plain, f"ran the {'PLAIN' if plain else 'general'} kernel"
    assert counts == o_counts, "ray counts differ"
    assert_same_pixels(rgba, o_rgba)


@pytest.mark.parametrize("mode", ["single", "pipelined"])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ["wall_z", "oblique", "spheres", "negative"])
def test_textured_frames(oracle_lib, example_scenes, name, w, h, mode):
    _check_frame(oracle_lib, name, _scenes(example_scenes)[name], w, h, mode)


@pytest.mark.parametrize("mode", ["single", "pipelined"])
@pytest.mark.parametrize("w,h", SIZES)
def test_test1_as_shipped(oracle_lib, example_scenes, w, h, mode):
    """The flagship scene: a textured floor (clay) and a textured sphere (land), three lights."""
    s = copy.deepcopy(example_scenes["test1"])
    s.max_recursion_depth = 5
    _check_frame(oracle_lib, "test1", s, w, h, mode)


# ---------------------------------------------------------------- 1/N shares
@pytest.mark.parametrize("mode", ["single", "pipelined"])
@pytest.mark.parametrize("tile_rows,stride,offset", [(8, 8, 0), (8, 8, 7), (3, 2, 1)])
def test_shares_equal_the_frames_rows(oracle_lib, example_scenes, tile_rows, stride, offset, mode):
    """Rank `offset` of `stride` ranks: row tiles offset, offset + stride, ... of the frame, dense in
    its buffer (rows past the frame's end are padding, zero).  (8, 8, 7) at 61 rows is the partial
    last tile alone; 3 rows per tile are no power of two."""
    w, h = 97, 61
    scene = _scenes(example_scenes)["spheres"]
    o_rgba, _ = oracle_frame(oracle_lib, "spheres", scene, w, h)
    t = _abi.rg_tiling(tile_rows, stride, offset)
    ds = DeviceScene(scene)
    rgba, _, plain, _ = device_launch(ds, w, h, mode, t)
    ds.close()
    assert plain, "a share must stay on the PLAIN kernel"
    tiles = list(range(offset, (h + tile_rows - 1) // tile_rows, stride))
    assert rgba.shape[0] == len(tiles) * tile_rows and tiles
    want = np.zeros_like(rgba)
    for k, ti in enumerate(tiles):
        n = min(tile_rows, h - ti * tile_rows)
        want[k * tile_rows:k * tile_rows + n] = o_rgba[ti * tile_rows:ti * tile_rows + n]
    assert_same_pixels(rgba, want)


# ---------------------------------------------------------------- the check refused
@pytest.mark.parametrize("mode", ["single", "pipelined"])
@pytest.mark.parametrize("w,h", SIZES)
def test_quotient_check_failed_takes_the_general_kernel(oracle_lib, example_scenes, w, h, mode):
    """No frame size up to 20000 pixels a side fails the quotient sweep (tests/test_exact_div.py), so
    the debug setter makes the launch context report one: general kernel, same bytes; switched on
    again, the same handle is back on the PLAIN kernel."""
    scene = _scenes(example_scenes)["oblique"]
    _check_frame(oracle_lib, "oblique", scene, w, h, mode, expect_plain=False, prepare=lambda ds: ds.set_exact_div(False))
    o_rgba, o_counts = oracle_frame(oracle_lib, "oblique", scene, w, h)
    ds = DeviceScene(scene)
    seen = []
    for enable in (False, True, False):
        ds.set_exact_div(enable)
        rgba, counts, plain, _ = device_launch(ds, w, h, mode)
        seen.append(plain)
        assert counts == o_counts and np.array_equal(rgba, o_rgba)
    ds.close()
    assert seen == [False, True, False]
