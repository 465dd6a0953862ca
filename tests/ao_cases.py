"""The parity cases of the ambient occlusion tests, shared by tests/test_ao_cpu.py (which checks the condition on
the inputs on the CPU) and tests/test_gpu_ao.py (which renders them).

A parity case proves little if every pixel is 0 or 1.  So for each scene and radius used at 97x61 the REFERENCE
must give at least 5 % of the hit pixels a value strictly between 0 and 1 -- at every k >= 2 the case is run with
(k = 1 gives 0 or 1 by construction) -- and with a finite radius it must differ from the +inf result in at least
one pixel.  The radii below were chosen on the CPU against that condition: each "cuts through the scene's
neighbours" (test1 - test3: 8, slab: 2, the synthetic scenes: 16 - 32 of their ~100 extent).

synth64 (64 spheres inside 8 planes, a closed room) is wholly occluded at +inf -- every ray ends on a wall, the
reference gives 0.0 everywhere -- so it is run with two finite radii, and `open64` (the same 64 spheres over 2
planes) carries +inf through the BVH flavours in its place.
"""
import numpy as np

import ao_ref
from raingun_amd.camera import Camera
from raingun_amd.color import Color
from raingun_amd.scene import DirectionalLight, Material, Plane, Scene, Sphere
from raingun_amd.synth import synthetic_scene

INF = float("inf")
W, H = 97, 61
SMALL = [(1, 1), (17, 3)]
# scene -> (the two radii of its cases)
RADII = {
    "test1": (INF, 8.0),
    "test2": (INF, 8.0),
    "test3": (INF, 8.0),
    "synth16": (INF, 32.0),
    "synth64": (24.0, 16.0),
    "open64": (INF, 24.0),
    "slab": (INF, 2.0),
}
SCENES = list(RADII)
BIASES = (1e-13, 1e-6)
MIN_PARTIAL = 0.05

_OWN = {}


def scene(example_scenes, name):
    """test_gpu_camera's scenes, plus open64."""
    from test_gpu_camera import _scene

    if name == "open64":
        if name not in _OWN:
            _OWN[name] = synthetic_scene(64, 2, 8)
        return _OWN[name]
    return _scene(example_scenes, name)


def combos(name):
    """(k, radius, bias): every k of {1, 2, 3, 8}, both radii of the scene and both biases, each met by a case;
    every path and BVH flavour runs all four."""
    r0, r1 = RADII[name]
    return [(1, r0, BIASES[0]), (2, r1, BIASES[1]), (3, r0, BIASES[1]), (8, r1, BIASES[0])]


def ref(example_scenes, name, w, h, k, radius=INF, bias=1e-13, cam=None, **tiling):
    return ao_ref.cached(name, scene(example_scenes, name), w, h, k, radius, bias, cam, **tiling)


def partial_share(ao, opened):
    """The share of the hit pixels whose value lies strictly between 0 and 1."""
    hit = opened >= 0
    return float(((ao > 0) & (ao < 1) & hit).sum()) / max(int(hit.sum()), 1)


def assert_condition(example_scenes, name):
    """The condition on the inputs, on the reference."""
    for k, radius, bias in combos(name):
        if k < 2:
            continue
        st, a, _, err, opened, _ = ref(example_scenes, name, W, H, k, radius, bias)
        assert st == 0 and err == -1, (name, k, radius)
        share = partial_share(a, opened)
        assert share >= MIN_PARTIAL, f"{name} k {k} radius {radius}: only {share:.3f} of the hit pixels are partial"
        if np.isfinite(radius):
            a_inf = ref(example_scenes, name, W, H, k, INF, bias)[1]
            assert (a != a_inf).any(), f"{name} k {k}: radius {radius} changes nothing"


def nan_scene():
    """A sphere at 5e154 (tests/test_gpu_host_paths.py _far_sphere_scene): for a ray with a large component
    towards it h.h and adj^2 overflow and opp = inf - inf is NaN (bodies.rs:95), so the sphere 'hits' at NaN, and
    Scene::trace panics (scene.rs:38) when the ray has another hit besides.  At fov 30 no primary ray does: they
    end on the floor or the ceiling with |d.y| small.  The AO rays of either leave it steeply enough for
    (5e154 d.y)^2 to overflow, and meet the other plane besides."""
    m = Material(Color.from_str("#ffffff"), 0.5)
    bodies = [Sphere((0.0, 5e154, 0.0), 1.0, m), Plane((0.0, -2.0, 0.0), (0.0, -1.0, 0.0), m),
              Plane((0.0, 10.0, 0.0), (0.0, 1.0, 0.0), m)]
    return Scene(fov=30.0, bodies=bodies, lights=[DirectionalLight((0.0, -1.0, 0.0), Color.from_str("#ffffff"), 1.0)])


CLI_CAMERA = Camera.look_at((3, 2, -10), (0, 0, -30))
