"""Seeded scenes that mix all four body kinds, shared by tests/test_mixed_scenes_cpu.py, tests/test_gpu_mixed.py
and tests/test_synth.py.  A plain module: everything follows from a seed through numpy.random.default_rng,
nothing is read from disk, and the two textures are small RGBA arrays made here.

mixed_scene() interleaves spheres, planes, disks and boxes in a seeded shuffle of the YAML order and gives the
bodies of each kind the six (surface, coloration) combinations in turn, so a scene with six bodies of a kind
has all six of that kind.  CONFIGS names the members of the family with the reason each one exists;
config_scene(name) builds one.  tests/test_mixed_scenes_cpu.py holds the conditions the family must meet
(every possible combination is the primary hit of some pixels, secondary and shadow rays exist), so that no
GPU test over it passes vacuously.  trace_rays(name) gives the rays of the Scene::trace comparison.
"""
from collections import namedtuple

import numpy as np

from raingun_amd.color import Color
from raingun_amd.scene import AABB, DirectionalLight, Disk, Material, Plane, Scene, Sphere, SphericalLight, Texture

KINDS = ("Sphere", "Plane", "Disk", "AABB")
SURFACES = ("Diffuse", "Reflecting", "Refractive")
# the six materials of a kind in round-robin order: (surface, textured)
COMBOS = tuple((s, t) for t in (False, True) for s in SURFACES)
ALL_COMBOS = tuple((k, s, t) for k in KINDS for s, t in COMBOS)  # the 24 of the family


def _texels(w, h):
    """(h, w, 4) RGBA whose every texel differs from its eight neighbours in R (steps of 29, 83, 112 and 54
    modulo 200), so a lookup that is one texel off changes the colour."""
    x = np.arange(w, dtype=np.int64)[None, :]
    y = np.arange(h, dtype=np.int64)[:, None]
    img = np.empty((h, w, 4), dtype=np.uint8)
    img[..., 0] = (x * 29 + y * 83) % 200 + 50
    img[..., 1] = (x * 97 + y * 41 + 7) % 200 + 50
    img[..., 2] = ((x + y) * 61) % 200 + 50
    img[..., 3] = 255
    return img


# two textures, neither size a power of two nor equal to the other's; offsets non-zero, one negative per texture
TEX_A = _texels(7, 5)
TEX_B = _texels(64, 33)
TEX_OFFSETS = {id(TEX_A): (0.25, -0.375), id(TEX_B): (-1.5, 0.625)}
for _t in (TEX_A, TEX_B):
    _t.setflags(write=False)

# one-sided planes (hit where dot(normal, direction) > 1e-6): floor, back wall, side walls, ceiling, one oblique
_S = 0.5 ** 0.5
PLANES = (((0.0, -3.0, 0.0), (0.0, -1.0, 0.0)),
          ((0.0, 0.0, -32.0), (0.0, 0.0, -1.0)),
          ((-10.0, 0.0, 0.0), (-1.0, 0.0, 0.0)),
          ((10.0, 0.0, 0.0), (1.0, 0.0, 0.0)),
          ((0.0, 7.0, 0.0), (0.0, 1.0, 0.0)),
          ((7.0, 0.0, -29.0), (_S, 0.0, -_S)))


def _material(rng, combo, textures):
    surface, textured = combo
    if textured:
        img = textures[int(rng.integers(2))]
        xo, yo = TEX_OFFSETS[id(img)]
        coloration = Texture("", img, xo, yo)
    else:
        coloration = Color(*(float(c) for c in rng.integers(3, 9, size=3) / 8.0))
    m = Material(coloration, float(rng.integers(5, 15)) / 16.0, surface)
    if surface == "Reflecting":
        m.reflectivity = float(rng.integers(3, 10)) / 16.0
    elif surface == "Refractive":
        m.index = float(rng.integers(21, 28)) / 16.0
        m.transparency = float(rng.integers(11, 16)) / 16.0
    return m


def _place(rng):
    """A point in front of the default camera, inside the 97x61 frustum: x in [-8, 8], y in [-2.5, 6], z in [-30, -4]."""
    z = -float(rng.uniform(5.0, 28.0))
    x = float(rng.uniform(-1.0, 1.0)) * min(8.0, 1.3 * -z)
    y = float(rng.uniform(max(-2.5, 0.8 * z), min(6.0, 0.8 * -z)))
    return x, y, z


def mixed_scene(seed, n_sph, n_pln, n_dsk, n_box, n_lights, depth):
    """The scene of one seed: n_sph spheres, n_pln planes (the first of PLANES), n_dsk disks and n_box boxes
    in a seeded shuffle, n_lights lights (one directional, then spherical ones), recursion depth `depth`."""
    assert 0 <= n_pln <= len(PLANES)
    rng = np.random.default_rng(seed)
    textures = (TEX_A, TEX_B)
    n_bodies = n_sph + n_pln + n_dsk + n_box
    size = min(1.0, (40.0 / max(n_bodies, 1)) ** 0.5)  # crowded scenes get smaller bodies
    start = [int(rng.integers(6)) for _ in KINDS]      # where each kind's round-robin starts

    def combo(kind, i):
        return COMBOS[(start[kind] + i) % 6]

    bodies = []
    for i in range(n_sph):
        x, y, z = _place(rng)
        bodies.append(Sphere((x, y, z), -z * size * float(rng.uniform(0.06, 0.12)), _material(rng, combo(0, i), textures)))
    for i in range(n_pln):
        bodies.append(Plane(PLANES[i][0], PLANES[i][1], _material(rng, combo(1, i), textures)))
    disks = []
    for i in range(n_dsk):
        x, y, z = _place(rng)
        if i % 4 == 0:
            n = (0.0, 0.0, -1.0)  # cross(n, unit_z) == 0: texture_coords takes the cross(n, unit_y) fallback
        else:                     # oblique, facing the camera: the view direction of the centre, tilted
            v = np.array([x, y, z]) / np.sqrt(x * x + y * y + z * z) + rng.uniform(-0.35, 0.35, size=3)
            v /= np.sqrt((v * v).sum())
            n = tuple(float(c) for c in v)
        disks.append(Disk((x, y, z), n, -z * size * float(rng.uniform(0.08, 0.15)), _material(rng, combo(2, i), textures)))
    boxes = []
    for i in range(n_box):
        x, y, z = _place(rng)
        hx, hy, hz = (-z * size * float(rng.uniform(0.05, 0.10)) for _ in range(3))
        boxes.append(AABB(((x - hx, y - hy, z - hz), (x + hx, y + hy, z + hz)), _material(rng, combo(3, i), textures)))
    bodies += disks + boxes
    order = rng.permutation(len(bodies))
    bodies = [bodies[int(k)] for k in order]

    lights = []
    if n_lights > 0:
        lights.append(DirectionalLight((0.3, -1.0, -0.5), Color(1.0, 0.95, 0.9), 1.5))
    spots = []
    if boxes:  # inside a box: every shadow ray towards it enters that box first
        lo, hi = boxes[0].bounds
        spots.append(tuple((a + b) / 2.0 for a, b in zip(lo, hi)))
    if disks:  # behind a disk, seen from the camera
        d = disks[0]
        spots.append(tuple(o + 1.5 * n for o, n in zip(d.origin, d.normal)))
    for i in range(max(n_lights - 1, 0)):
        pos = spots[i] if i < len(spots) else (float(rng.uniform(-7.0, 7.0)), float(rng.uniform(3.0, 6.0)),
                                               float(rng.uniform(-24.0, -3.0)))
        col = Color(*(float(c) for c in rng.integers(5, 9, size=3) / 8.0))
        lights.append(SphericalLight(pos, col, float(rng.integers(8, 25)) * 250.0))
    return Scene(fov=90.0, default_color=Color(0.125, 0.25, 0.375), max_recursion_depth=depth, bodies=bodies,
                 lights=lights)


# a refractive box around the default camera: every primary ray starts inside it (aabb_hit's tmax branch)
ENCLOSING_BOX = ((-1.5, -1.0, -2.0), (1.25, 1.5, 0.75))


def enclose_camera(scene):
    m = Material(Color(0.875, 1.0, 0.9375), 0.5, "Refractive", index=1.5, transparency=0.9375)
    scene.bodies.append(AABB(ENCLOSING_BOX, m))
    return scene


Config = namedtuple("Config", "seed n_sph n_pln n_dsk n_box n_lights depth inside", defaults=(False,))

# The seeds are the first ones (counting up from 1) with which the config meets the conditions of
# tests/test_mixed_scenes_cpu.py; RG_BVH_MIN_SPHERES is 16, RG_HEAVY_SCENE_BODIES 32, RG_LB (the light
# kernels' light count) 3.
CONFIGS = {
    # light path, the 3-light shadow batch, the d8 kernels, never PLAIN
    "light3": Config(1, 5, 2, 3, 3, 3, 5),
    # the 2-light shadow batch and the d64 kernels
    "light2_d64": Config(1, 3, 1, 1, 1, 2, 20),
    # one light, the d16 kernels, 15 spheres (one short of a BVH), 31 bodies (one under the heavy threshold)
    "light1_d16": Config(16, 15, 2, 9, 5, 1, 12),
    # no lights: no shadow rays at all
    "light0": Config(1, 4, 1, 2, 2, 0, 3),
    # the d0 kernels: primary rays only
    "d0": Config(1, 5, 2, 3, 3, 3, 0),
    # an odd sphere count with a BVH built, 31 bodies: auto = light; forced heavy = BVH walk + linear disks / boxes
    "bvh17": Config(8, 17, 3, 5, 6, 3, 8),
    # exactly 32 bodies: auto = heavy; 16 spheres, the smallest BVH
    "heavy32": Config(5, 16, 4, 6, 6, 3, 5),
    # more lights than the light kernels take, so auto = heavy; light buffers with non-sphere occluders; odd count
    "heavy5l": Config(4, 33, 6, 7, 9, 5, 5),
    # more disks and boxes than any shipped scene
    "many": Config(3, 64, 2, 16, 16, 3, 5),
    # empty sphere tables on both paths
    "nosph": Config(1, 0, 1, 12, 12, 2, 6),
    # light3 inside a refractive box: the tmax branch on every primary ray, transmission out of a box
    "inside_box": Config(1, 5, 2, 3, 3, 3, 5, True),
}

_SCENES = {}


def config_scene(name):
    """The scene of CONFIGS[name], built once (the tests share it and leave it unchanged)."""
    if name not in _SCENES:
        c = CONFIGS[name]
        s = mixed_scene(*c[:7])
        _SCENES[name] = enclose_camera(s) if c.inside else s
    return _SCENES[name]


def combo_of(body):
    """(kind, surface, textured) of a body: one of ALL_COMBOS."""
    kind = {Sphere: "Sphere", Plane: "Plane", Disk: "Disk", AABB: "AABB"}[type(body)]
    return kind, body.material.surface, isinstance(body.material.coloration, Texture)


def possible_combos(name):
    """The combinations that can be a primary hit in CONFIGS[name]: those of its bodies, or, when a box
    encloses the camera, that box's alone."""
    bodies = config_scene(name).bodies
    if CONFIGS[name].inside:
        return {combo_of(bodies[-1])}
    return {combo_of(b) for b in bodies}


def primary_hit_counts(name, body_layer):
    """{combination: pixels} of an AOV `body` layer of CONFIGS[name]."""
    bodies = config_scene(name).bodies
    per_body = np.bincount(body_layer[body_layer >= 0].ravel(), minlength=len(bodies))
    out = {c: 0 for c in ALL_COMBOS}
    for b, n in zip(bodies, per_body):
        out[combo_of(b)] += int(n)
    return out


def trace_rays(name, n=4096, seed=77):
    """(n, 6) rays for Scene::trace on CONFIGS[name], and how many of the last ones are rim rays.

    A third start anywhere in the scene's extent, a third inside a box (the slab test's tmax branch), a third
    are aimed at a body's centre.  One ray in eight has a direction component of exactly 0.0 and one in eight
    of -0.0: infinite reciprocals of either sign in the slab test, and no NaN, since no origin lies in a slab
    plane.  The rim rays fall straight onto the disks whose normal is (0, 0, -1) at a point whose distance from
    the centre, as bodies.rs computes it, equals the radius exactly: `<` misses there and `<=` would hit."""
    scene = config_scene(name)
    rng = np.random.default_rng(seed)
    boxes = [b for b in scene.bodies if isinstance(b, AABB)]
    o = np.stack([rng.uniform(-9.0, 9.0, n), rng.uniform(-2.5, 6.5, n), rng.uniform(-31.0, 1.0, n)], axis=1)
    d = rng.normal(size=(n, 3))
    for i in range(n):
        if i % 3 == 1 and boxes:
            lo, hi = (np.array(c) for c in boxes[int(rng.integers(len(boxes)))].bounds)
            o[i] = lo + rng.uniform(0.05, 0.95, 3) * (hi - lo)
        elif i % 3 == 2:
            b = scene.bodies[int(rng.integers(len(scene.bodies)))]
            c = np.array(b.center if isinstance(b, Sphere) else np.add(*b.bounds) / 2.0 if isinstance(b, AABB) else b.origin)
            d[i] = c + rng.uniform(-0.5, 0.5, 3) - o[i]
        if i % 8 == 0:
            d[i, int(rng.integers(3))] = 0.0
        elif i % 8 == 4:
            d[i, int(rng.integers(3))] = -0.0
    d /= np.sqrt((d * d).sum(axis=1, keepdims=True))
    rim = []
    for b in scene.bodies:
        if not (isinstance(b, Disk) and b.normal == (0.0, 0.0, -1.0)):
            continue
        ox, oy, oz = b.origin
        for ux, uy in ((1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0)):
            for back in (1.0, 2.0, 3.0, 4.0, 0.5):
                px, py, pz = ox + ux * b.radius, oy + uy * b.radius, oz + back
                dist = ((ox - px) * 0.0 + (oy - py) * 0.0) + (oz - pz) * -1.0   # bodies.rs:176-177, den == 1
                w = ((px + 0.0 * dist) - ox, (py + 0.0 * dist) - oy, (pz + -1.0 * dist) - oz)
                if dist >= 0.0 and float(np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])) == b.radius:
                    rim.append((px, py, pz, 0.0, 0.0, -1.0))
                    break
    rays = np.concatenate([o, d], axis=1)
    if rim:
        rays[n - len(rim):] = np.array(rim)
    return rays, len(rim)
