"""Scenes in which two or more bodies lie at bit-equal distance along many rays, shared by
tests/test_tie_scenes_cpu.py and tests/test_gpu_ties.py.  A plain module in the style of tests/mixed_scenes.py:
seeded, nothing read from disk, every scene built once and handed out unchanged.

Scene::trace keeps the first minimum in YAML order (scene.rs:34-39).  The device regroups the bodies by kind
and permutes the spheres into BVH leaf order, so every closest-hit path rebuilds that rule from a carried id
(closest_add, raingun_amd/csrc/rg_k_intersect.h), and the BVH walk must not prune a child whose entry distance
equals the current best.  In seeded-random geometry no two bodies are ever at bit-equal distance; here they are:

with_twins(scene)   every body gets a twin of the same geometry (so of the same arithmetic, bit for bit) with
                    another surface kind and another colour, or the other texture.  The twins of the
                    odd-indexed bodies come before all the originals, those of the even-indexed ones after them
                    in reverse: in about half the ties the winner is listed late in its kind's device table.
coplanar_scene()    hand-written, every coordinate dyadic: box faces and disks in the floor and in the back
                    wall, the floor a second time from another origin with an unnormalised normal, a sphere
                    resting on the floor, touching and concentric spheres, a box in a box sharing a face, and
                    lights inside the inner box, just above the coplanar patch and exactly in the back wall
                    (a shadow ray towards that one meets the wall at the light's own distance, to the last bit
                    or one ulp off it either way).
limits_scene()      the ends of every material range and a light of intensity 0, no ties.

tests/test_tie_scenes_cpu.py holds the conditions that keep the GPU tests from passing vacuously.
"""
import copy
from collections import namedtuple

import numpy as np

from mixed_scenes import TEX_A, TEX_B, TEX_OFFSETS, mixed_scene
from raingun_amd.color import Color
from raingun_amd.scene import AABB, DirectionalLight, Disk, Material, Plane, Scene, Sphere, SphericalLight, Texture

SURFACES = ("Diffuse", "Reflecting", "Refractive")


def _texture(img):
    xo, yo = TEX_OFFSETS[id(img)]
    return Texture("", img, xo, yo)


def _twin_material(rng, m, other_texture):
    """Another surface kind than m's, and another plain colour, or (other_texture) the other texture."""
    surface = SURFACES[(SURFACES.index(m.surface) + 1 + int(rng.integers(2))) % 3]
    if other_texture:
        coloration = _texture(TEX_B if m.coloration.image is TEX_A else TEX_A)
    else:
        while True:
            coloration = Color(*(float(c) for c in rng.integers(2, 9, size=3) / 8.0))
            if isinstance(m.coloration, Texture) or coloration != m.coloration:
                break
    t = Material(coloration, float(rng.integers(5, 15)) / 16.0, surface)
    if surface == "Reflecting":
        t.reflectivity = float(rng.integers(3, 10)) / 16.0
    elif surface == "Refractive":
        t.index = float(rng.integers(21, 28)) / 16.0
        t.transparency = float(rng.integers(11, 16)) / 16.0
    return t


def twins_of(bodies, seed):
    """One twin per body, in the bodies' order: the same geometry, another material.  Every second textured
    original keeps a textured twin (the other texture): there a wrong winner changes the texel."""
    rng = np.random.default_rng(seed)
    out, textured = [], 0
    for b in bodies:
        is_tex = isinstance(b.material.coloration, Texture)
        t = copy.copy(b)
        t.material = _twin_material(rng, b.material, is_tex and textured % 2 == 0)
        textured += int(is_tex)
        out.append(t)
    return out


def arrange(bodies, twins):
    """Twins of the odd-indexed bodies, then all the originals, then the twins of the even-indexed ones reversed."""
    return twins[1::2] + list(bodies) + twins[0::2][::-1]


def with_twins(scene, seed=1):
    """A copy of `scene` in which every body has a twin (twins_of, arrange)."""
    s = copy.copy(scene)
    s.bodies = arrange(scene.bodies, twins_of(scene.bodies, seed))
    return s


def reversed_bodies(scene):
    """The same scene with its body list reversed: every exact tie goes to the other body."""
    s = copy.copy(scene)
    s.bodies = list(scene.bodies)[::-1]
    return s


# ---------------------------------------------------------------- the hand-written scenes
def _col(r, g, b):
    return Color(r / 8.0, g / 8.0, b / 8.0)


def _diffuse(c, albedo=0.5):
    return Material(c, albedo, "Diffuse")


def _mirror(c, reflectivity=0.5, albedo=0.5):
    return Material(c, albedo, "Reflecting", reflectivity=reflectivity)


def _glass(c, index=1.5, transparency=0.875, albedo=0.5):
    return Material(c, albedo, "Refractive", index=index, transparency=transparency)


FLOOR_Y, WALL_Z = -3.0, -32.0
# where bodies coincide, for trace_rays: (x0, x1, z0, z1) on the floor, (x0, x1, y0, y1) on the back wall
FLOOR_PATCH = (-5.0, 6.0, -15.0, -7.0)
WALL_PATCH = (-9.0, 10.0, -1.0, 7.0)
LIGHT_IN_WALL = (12.0, 8.0, WALL_Z)
COPLANAR_FLOOR = (0, 1, 2, 3, 4, 16)   # the bodies of coplanar_scene() that lie in the floor plane ...
COPLANAR_WALL = (5, 6, 7, 8)           # ... and in the back wall


def coplanar_scene():
    """Every coordinate, radius and normal is a dyadic rational of few bits, so the construction is exact: the
    bodies named coplanar ARE coplanar in f64, and what is left to rounding is the hit distance alone (a plane
    or disk divides by dot(n, d), a box multiplies by 1 / d.y: equal or one ulp apart)."""
    up, front = (0.0, -1.0, 0.0), (0.0, 0.0, -1.0)  # one-sided: hit where dot(normal, direction) > 1e-6
    bodies = [
        Disk((2.0, FLOOR_Y, -10.0), up, 1.5, _mirror(_col(8, 2, 2), 0.375)),            # 0 in the floor, on the box top, first
        Plane((0.0, FLOOR_Y, 0.0), up, _diffuse(_texture(TEX_B))),                      # 1 the floor
        AABB(((0.0, -5.0, -14.0), (4.0, FLOOR_Y, -8.0)), _diffuse(_col(2, 8, 2))),      # 2 sunk: its top is in the floor
        Plane((5.0, FLOOR_Y, -7.0), (0.0, -4.0, 0.0), _mirror(_col(2, 2, 8), 0.25)),    # 3 the floor again: |n| = 4
        Disk((-3.0, FLOOR_Y, -9.0), up, 1.5, _glass(_col(8, 8, 2))),                    # 4 in the floor, after both planes
        Disk((6.0, 2.0, WALL_Z), front, 3.0, _mirror(_col(7, 1, 7), 0.625)),            # 5 in the back wall, before it
        Plane((0.0, 0.0, WALL_Z), front, _diffuse(_texture(TEX_A))),                    # 6 the back wall
        AABB(((-8.0, 0.0, -36.0), (-2.0, 6.0, WALL_Z)), _mirror(_col(8, 4, 1), 0.5)),   # 7 its front is in the back wall
        Disk((-5.0, 3.0, WALL_Z), front, 2.0, _diffuse(_col(1, 6, 8))),                 # 8 in the wall, on the box front, last
        Sphere((-1.0, -2.0, -11.0), 1.0, _mirror(_col(8, 8, 8), 0.75)),                 # 9 rests on the floor at (-1, -3, -11)
        Sphere((-4.0, 0.0, -16.0), 1.0, _diffuse(_col(8, 3, 3))),                       # 10 touches 11 at (-3, 0, -16)
        Sphere((-2.0, 0.0, -16.0), 1.0, _glass(_col(3, 8, 3), 1.25)),                   # 11
        Sphere((4.0, 1.0, -14.0), 1.5, _glass(_col(7, 8, 8), 1.5, 0.9375)),             # 12 the outer of two concentric spheres
        Sphere((4.0, 1.0, -14.0), 1.0, _diffuse(_col(8, 5, 0))),                        # 13 the inner one
        AABB(((-7.0, -2.0, -24.0), (-3.0, 2.0, -20.0)), _glass(_col(6, 7, 8), 1.5)),    # 14 a box ...
        AABB(((-6.0, -1.0, -22.0), (-4.0, 1.0, -20.0)), _glass(_col(8, 6, 7), 1.25)),   # 15 ... and one inside it, sharing z = -20
        Disk((4.0, FLOOR_Y, -12.0), up, 1.5, _diffuse(_col(4, 1, 6))),                  # 16 in the floor, across the box top's edge
    ]
    lights = [SphericalLight((-5.0, 0.0, -21.0), Color(1.0, 0.9375, 0.875), 3000.0),    # inside the inner box
              SphericalLight((2.0, -2.5, -10.0), Color(0.875, 1.0, 1.0), 1500.0),       # just above the coplanar patch
              SphericalLight(LIGHT_IN_WALL, Color(1.0, 1.0, 0.875), 9000.0)]            # exactly in the back wall
    return Scene(fov=90.0, default_color=Color(0.125, 0.25, 0.375), max_recursion_depth=5, bodies=bodies, lights=lights)


# the sphere of coplanar_bvh_scene() with a light exactly on its surface, and that light
LIT_SPHERE = ((8.0, 3.0, -20.0), 1.0)
LIGHT_ON_SPHERE = (7.0, 3.0, -20.0)


def coplanar_bvh_scene(seed=3):
    """coplanar_scene() plus 17 spheres on a 1/8 grid, ten of them twinned: 32 spheres (a BVH), 44 bodies (the
    heavy path by itself), and a fourth light exactly on a sphere's surface, so that the BVH leaves and the
    light buffers decide shadow rays at the light's own distance too."""
    s = coplanar_scene()
    rng = np.random.default_rng(seed)
    extra = [Sphere(LIT_SPHERE[0], LIT_SPHERE[1], _diffuse(_col(8, 7, 5)))]
    for i in range(16):
        z = -float(rng.integers(5 * 8, 28 * 8)) / 8.0
        x = float(rng.integers(-8, 9)) / 8.0 * min(8.0, -z)
        y = float(rng.integers(-2 * 8, 5 * 8)) / 8.0
        m = [_diffuse, _mirror, _glass][i % 3](_col(*(int(c) for c in rng.integers(2, 9, size=3))))
        extra.append(Sphere((x, y, z), float(rng.integers(3, 9)) / 8.0, m))
    twins = twins_of(extra[1:11], seed)
    s.bodies = twins[1::2] + s.bodies + extra + twins[0::2][::-1]
    s.lights = s.lights + [SphericalLight(LIGHT_ON_SPHERE, Color(1.0, 0.875, 0.75), 2500.0)]
    return s


def limits_scene():
    """Reflectivity 0 and 1, transparency 0 and 1, refractive index 0.5, 1.0 and 2.5, albedo 0 and 1, a light
    of intensity 0: the ends of the ranges, where the mixed family draws every parameter strictly inside."""
    up, front = (0.0, -1.0, 0.0), (0.0, 0.0, -1.0)
    bodies = [
        Plane((0.0, FLOOR_Y, 0.0), up, _mirror(_texture(TEX_B), 0.0, albedo=1.0)),
        Plane((0.0, 0.0, WALL_Z), front, _diffuse(_col(8, 8, 8), albedo=0.0)),
        Sphere((-6.0, -1.0, -12.0), 2.0, _mirror(_col(8, 8, 8), 1.0, albedo=1.0)),
        Sphere((-1.5, -1.5, -9.0), 1.5, _mirror(_col(8, 2, 2), 0.0, albedo=0.0)),
        Sphere((2.5, -1.0, -10.0), 2.0, _glass(_col(8, 8, 8), 0.5, 1.0)),
        Sphere((7.0, 0.0, -13.0), 2.0, _glass(_col(2, 8, 4), 1.0, 0.0, albedo=1.0)),
        Sphere((0.0, 3.5, -14.0), 2.0, _glass(_col(8, 8, 8), 2.5, 1.0, albedo=0.0)),
        Sphere((-4.0, 4.0, -18.0), 2.0, _glass(_texture(TEX_A), 1.0, 1.0)),
        Disk((5.0, 4.0, -16.0), (-0.25, -0.25, -1.0), 2.0, _mirror(_col(8, 8, 0), 1.0, albedo=0.0)),
        AABB(((-9.0, -2.5, -22.0), (-5.0, 0.5, -19.0)), _glass(_col(8, 4, 8), 2.5, 0.0, albedo=1.0)),
        AABB(((3.0, -2.75, -7.0), (5.0, -1.75, -5.0)), _mirror(_col(0, 0, 0), 1.0)),
    ]
    lights = [DirectionalLight((0.25, -1.0, -0.5), Color(1.0, 1.0, 1.0), 1.5),
              SphericalLight((0.0, 5.0, -8.0), Color(1.0, 0.5, 0.25), 0.0),
              SphericalLight((-3.0, 6.0, -6.0), Color(0.0, 1.0, 1.0), 4000.0)]
    return Scene(fov=90.0, default_color=Color(0.0, 0.0, 1.0), max_recursion_depth=6, bodies=bodies, lights=lights)


# ---------------------------------------------------------------- the configs
# mixed: the arguments of mixed_scenes.mixed_scene(seed, n_sph, n_pln, n_dsk, n_box, n_lights, depth) before
# twinning, or None for a hand-written scene.  RG_BVH_MIN_SPHERES is 16, RG_HEAVY_SCENE_BODIES 32, RG_LB (the
# light kernels' light count) 3.
Config = namedtuple("Config", "mixed twinned coplanar")

CONFIGS = {
    # spheres and planes only, 12 spheres and 16 bodies after twinning, 3 lights: the only config a PLAIN light
    # kernel may run (its first-hit tiles and its shadow mask volume decide between twins too); seed 3 is the first
    # with which some 8x8 tiles, and not all, show only Diffuse winners and so take the first-hit path
    "plain_twins": Config((3, 6, 2, 0, 0, 3, 5), True, False),
    # all four kinds on the light path's general kernels: 8 spheres (no BVH) and 24 bodies after twinning, the
    # 2-light shadow batch; pln_id, dsk_id and box_id on both paths' linear scans
    "light_twins": Config((1, 4, 2, 3, 3, 2, 5), True, False),
    # 8 spheres and their 8 twins: the smallest BVH, and both members of every pair are in it; 28 bodies, so the
    # light path by itself and the BVH only where the heavy path is forced
    "bvh16_twins": Config((1, 8, 2, 2, 2, 3, 5), True, False),
    # 17 spheres before twinning (an odd count), 56 bodies, 3 lights: the heavy path by itself, with the light
    # buffers and the camera buffer handing out RgSphF2::id
    "heavy_twins": Config((1, 17, 3, 4, 4, 3, 5), True, False),
    # more lights than a light kernel takes: the heavy path only; 18 spheres, 34 bodies
    "heavy5l_twins": Config((1, 9, 2, 3, 3, 5, 5), True, False),
    # ties across kinds and one-ulp near-ties, on the linear scans of both paths
    "coplanar": Config(None, False, True),
    # the same beside a BVH: a plane, disk or box hit bounds the walk at a distance a sphere may equal
    "coplanar_bvh": Config(None, False, True),
    # the material and light extremes; no ties
    "limits": Config(None, False, False),
}
TWINNED = [n for n, c in CONFIGS.items() if c.twinned]
COPLANAR = [n for n, c in CONFIGS.items() if c.coplanar]
_HAND = {"coplanar": coplanar_scene, "coplanar_bvh": coplanar_bvh_scene, "limits": limits_scene}

_SCENES = {}


def config_scene(name):
    """The scene of CONFIGS[name], built once (the tests share it and leave it unchanged)."""
    if name not in _SCENES:
        c = CONFIGS[name]
        _SCENES[name] = with_twins(mixed_scene(*c.mixed), c.mixed[0]) if c.mixed else _HAND[name]()
    return _SCENES[name]


def counts(name):
    """(spheres, planes, disks, boxes) of the config's scene."""
    kinds = [type(b) for b in config_scene(name).bodies]
    return tuple(kinds.count(k) for k in (Sphere, Plane, Disk, AABB))


def _aim_point(rng, body):
    """A point of (or near) the body to aim a ray at."""
    if isinstance(body, Sphere):
        return np.array(body.center) + rng.uniform(-0.6, 0.6, 3) * body.radius
    if isinstance(body, AABB):
        lo, hi = (np.array(c) for c in body.bounds)
        return lo + rng.uniform(0.0, 1.0, 3) * (hi - lo)
    r = getattr(body, "radius", 6.0)
    return np.array(body.origin) + rng.uniform(-0.6, 0.6, 3) * r


_RAYS = {}


def trace_rays(name, n=4096, seed=91):
    """(n, 6) rays for Scene::trace on CONFIGS[name], read-only.  Every ray is aimed at a point of a body (for
    the coplanar configs every second one at a point of the patches where bodies coincide); ray i starts at the
    origin for i % 4 == 0, inside the scene's extent for 1, some 100 units out for 2 and some 2000 units out
    for 3 (the BVH walk's far-origin shift)."""
    if name in _RAYS:
        return _RAYS[name]
    scene = config_scene(name)
    rng = np.random.default_rng(seed)
    rays = np.zeros((n, 6))
    for i in range(n):
        if CONFIGS[name].coplanar and i % 2 == 1:
            if i % 4 == 1:
                x0, x1, z0, z1 = FLOOR_PATCH
                target = np.array([rng.uniform(x0, x1), FLOOR_Y, rng.uniform(z0, z1)])
            else:
                x0, x1, y0, y1 = WALL_PATCH
                target = np.array([rng.uniform(x0, x1), rng.uniform(y0, y1), WALL_Z])
        else:
            target = _aim_point(rng, scene.bodies[int(rng.integers(len(scene.bodies)))])
        if i % 4 == 0:
            o = np.zeros(3)
        elif i % 4 == 1:
            o = np.array([rng.uniform(-9.0, 9.0), rng.uniform(-2.5, 6.5), rng.uniform(-31.0, 1.0)])
        else:  # above the floor and in front of the back wall, so that the one-sided planes are seen
            v = rng.normal(size=3)
            v[1], v[2] = abs(v[1]), abs(v[2])
            o = target + v / np.sqrt((v * v).sum()) * (100.0 if i % 4 == 2 else 2000.0)
        d = target - o
        rays[i, :3], rays[i, 3:] = o, d / np.sqrt((d * d).sum())
    rays.setflags(write=False)
    _RAYS[name] = rays
    return rays


def first_hit_tiles(scene, body_layer):
    """The 8x8 tiles of an AOV `body` layer whose pixels all show a miss or a Diffuse body, as a boolean array:
    the tiles that a PLAIN light kernel finishes on its first-hit path (max_recursion_depth > 1)."""
    assert scene.max_recursion_depth > 1
    simple = np.array([b.material.surface == "Diffuse" for b in scene.bodies] + [True])[body_layer]
    h, w = simple.shape
    pad = np.ones(((h + 7) // 8 * 8, (w + 7) // 8 * 8), dtype=bool)
    pad[:h, :w] = simple
    return pad.reshape(pad.shape[0] // 8, 8, pad.shape[1] // 8, 8).all(axis=(1, 3))


def kind_of(body):
    return {Sphere: 0, Plane: 1, Disk: 2, AABB: 3}[type(body)]
