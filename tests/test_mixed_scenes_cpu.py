"""The mixed-primitive scene family (tests/mixed_scenes.py) on the CPU (no GPU needed).

(a) The conditions the family must meet so that no GPU test over it passes vacuously, checked with the
    pinned oracle and the AOV reference (tests/aov_ref.py) at 97x61.  A seed that misses one is replaced in
    mixed_scenes.CONFIGS; the conditions stay.
(b) Determinism: two calls give byte-identical SceneDesc tables.
(c) An independent restatement of the primary hit in numpy f64, written from the reference's bodies.rs and
    material.rs in their expression order (not from oracle/raingun_oracle.c): intersect of the four kinds,
    the first minimum in YAML order, the normals (the box's face search in its order with the 1e-8 test),
    texture_coords of the four kinds, and the colour through Texture::wrap and the texel.  It is compared
    with the AOV reference's five layers on every config at 97x61 and 64x40, which pins the oracle on the
    disk and box features the three golden frames do not reach.
"""
import ctypes as C
import math

import numpy as np
import pytest

import aov_ref
import mixed_scenes
from mixed_scenes import ALL_COMBOS, CONFIGS, config_scene
from raingun_amd import aov
from raingun_amd.scene import AABB, Disk, Plane, SceneDesc, Sphere, Texture

W, H = 97, 61
SIZES = [(97, 61), (64, 40)]
F32 = np.float32
PI_F32 = F32(math.pi)  # std::f32::consts::PI


def _layers(name, w, h):
    return aov_ref.cached(("mixed", name), config_scene(name), w, h)


# ---------------------------------------------------------------- (a) the family's conditions
@pytest.mark.parametrize("name", list(CONFIGS))
def test_config_meets_the_conditions(oracle_lib, name):
    cfg, scene = CONFIGS[name], config_scene(name)
    st, _, _, counts, err = oracle_lib.render(SceneDesc(scene), W, H)
    assert st == 0 and err == -1
    a_st, layers, a_counts, a_err = _layers(name, W, H)
    assert a_st == 0 and a_err == -1 and a_counts["primary"] == counts["primary"] == W * H
    kinds = [type(b) for b in scene.bodies]
    assert [kinds.count(k) for k in (Sphere, Plane, Disk, AABB)] == [cfg.n_sph, cfg.n_pln, cfg.n_dsk,
                                                                     cfg.n_box + (1 if cfg.inside else 0)]
    assert len(scene.lights) == cfg.n_lights and scene.max_recursion_depth == cfg.depth
    hits = mixed_scenes.primary_hit_counts(name, layers["body"])
    print(name, {f"{k} {s} {'tex' if t else 'col'}": n for (k, s, t), n in hits.items() if n})
    for combo in mixed_scenes.possible_combos(name):
        assert hits[combo] >= 8, f"{name}: {combo} is the primary hit of {hits[combo]} pixels"
    assert (counts["secondary"] > 0) == (cfg.depth > 0)
    assert (counts["shadow"] > 0) == (cfg.n_lights > 0)
    if cfg.inside:
        assert (layers["body"] == len(scene.bodies) - 1).all(), "a primary ray leaves the enclosing box unseen"


def test_family_covers_all_24_combinations():
    total = {c: 0 for c in ALL_COMBOS}
    for name in CONFIGS:
        for c, n in mixed_scenes.primary_hit_counts(name, _layers(name, W, H)[1]["body"]).items():
            total[c] += n
    assert len(total) == 24
    for c, n in total.items():
        assert n >= 100, f"{c} is the primary hit of {n} pixels over the whole family"


def test_generator_properties():
    """What mixed_scenes.py promises of the generator itself, on the largest mix: disks facing down -z, all six
    materials of a kind, an interleaved YAML order, the two textures, and where the spherical lights sit."""
    s = config_scene("many")
    disks = [b for b in s.bodies if isinstance(b, Disk)]
    assert 4 * sum(d.normal == (0.0, 0.0, -1.0) for d in disks) >= len(disks)
    assert all(d.normal[2] < 0.0 for d in disks)
    for kind in (Sphere, Disk, AABB):  # >= 6 of a kind: all six materials
        assert len({mixed_scenes.combo_of(b)[1:] for b in s.bodies if isinstance(b, kind)}) == 6
    assert len({mixed_scenes.combo_of(b)[1:] for b in config_scene("heavy5l").bodies if isinstance(b, Plane)}) == 6
    kinds = [type(b) for b in s.bodies]
    assert kinds != sorted(kinds, key=[Sphere, Plane, Disk, AABB].index), "the YAML order is grouped by kind"
    texs = {id(b.material.coloration.image): b.material.coloration for b in s.bodies
            if isinstance(b.material.coloration, Texture)}
    assert len(texs) == 2
    shapes = sorted(t.image.shape[:2] for t in texs.values())
    assert shapes == [(5, 7), (33, 64)]
    assert all(t.x_offset != 0 and t.y_offset != 0 and min(t.x_offset, t.y_offset) < 0 for t in texs.values())
    for t in texs.values():  # a one-texel error changes the colour
        img = t.image.astype(np.int32)
        for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
            a = img[max(dy, 0):, max(dx, 0):img.shape[1] + min(dx, 0), :3]
            b = img[:img.shape[0] - dy, max(-dx, 0):img.shape[1] - max(dx, 0), :3]
            assert (a != b).any(axis=2).all()
    # one spherical light inside a box, one behind a disk
    inside = [any(all(l < p < h for l, p, h in zip(b.bounds[0], light.position, b.bounds[1]))
                  for b in s.bodies if isinstance(b, AABB)) for light in s.lights[1:]]
    assert inside[0] and hasattr(s.lights[0], "direction")
    behind = s.lights[2].position
    assert any(all(abs(o + 1.5 * n - p) < 1e-12 for o, n, p in zip(d.origin, d.normal, behind)) for d in disks)


# ---------------------------------------------------------------- (b) determinism
def _table_bytes(desc):
    d = desc.desc
    out = [C.string_at(d.bodies, d.n_bodies * C.sizeof(desc.bodies[0])), C.string_at(d.lights, d.n_lights * C.sizeof(desc.lights[0]))]
    for i in range(d.n_textures):
        t = d.textures[i]
        out.append(bytes([t.width % 256, t.height % 256]) + C.string_at(t.rgba, t.width * t.height * 4))
    return out


@pytest.mark.parametrize("name", ["many", "inside_box", "nosph"])
def test_deterministic(name):
    c = CONFIGS[name]
    a, b = (mixed_scenes.mixed_scene(*c[:7]) for _ in range(2))
    if c.inside:
        a, b = mixed_scenes.enclose_camera(a), mixed_scenes.enclose_camera(b)
    da, db = SceneDesc(a), SceneDesc(b)
    assert a is not b and _table_bytes(da) == _table_bytes(db) == _table_bytes(SceneDesc(config_scene(name)))
    assert (da.desc.fov, da.desc.max_recursion_depth, list(da.desc.default_color)) == \
           (db.desc.fov, db.desc.max_recursion_depth, list(db.desc.default_color))
    other = SceneDesc(mixed_scenes.mixed_scene(c.seed + 1, *c[1:7]))
    assert _table_bytes(other)[0] != _table_bytes(da)[0]


# ---------------------------------------------------------------- (c) the primary hit, restated from bodies.rs
def _dot(a, b):  # cgmath: (x x' + y y') + z z'
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _intersect(body, o, d, inv, sign):
    """Option<f64> over all pixels: (hit mask, distance)."""
    with np.errstate(all="ignore"):
        if isinstance(body, Sphere):  # bodies.rs:76-120
            hyp = _sub(body.center, o)
            adj = _dot(hyp, d)
            opp2 = _dot(hyp, hyp) - (adj * adj)
            r2 = body.radius * body.radius
            some = ~(opp2 > r2)
            thick = np.sqrt(r2 - opp2)
            d0, d1 = adj - thick, adj + thick
            some &= ~((d0 < 0.0) & (d1 < 0.0))
            t = np.where(d0 < 0.0, d1, np.where(d1 < 0.0, d0, np.minimum(d0, d1)))
            return some, t
        if isinstance(body, (Plane, Disk)):  # bodies.rs:136-149, 173-192
            den = _dot(body.normal, d)
            v = _sub(body.origin, o)
            t = _dot(v, body.normal) / den
            some = (den > 1e-6) & (t >= 0.0)
            if isinstance(body, Disk):
                hit = tuple(o[k] + d[k] * t for k in range(3))
                w = _sub(hit, body.origin)
                some &= np.sqrt(_dot(w, w)) < body.radius
            return some, t
        lo, hi = body.bounds  # bodies.rs:242-282

        def slab(k):
            near = np.where(sign[k] == 1, hi[k], lo[k])  # bounds[sign]
            far = np.where(sign[k] == 1, lo[k], hi[k])   # bounds[1 - sign]
            return (near - o[k]) * inv[k], (far - o[k]) * inv[k]

        tmin, tmax = slab(0)
        tymin, tymax = slab(1)
        some = ~((tmin > tymax) | (tymin > tmax))
        tmin = np.where(tymin > tmin, tymin, tmin)
        tmax = np.where(tymax < tmax, tymax, tmax)
        tzmin, tzmax = slab(2)
        some &= ~((tmin > tzmax) | (tzmin > tmax))
        tmin = np.where(tzmin > tmin, tzmin, tmin)
        tmax = np.where(tzmax < tmax, tzmax, tmax)
        some &= (tmin >= 0.0) | (tmax >= 0.0)
        return some, np.where(tmin >= 0.0, tmin, tmax)


def _wrap(val, size):  # material.rs:70-79: `as i32` truncates and saturates, % keeps the dividend's sign
    fc = (val * F32(size)).astype(np.float64)
    i = np.where(np.isnan(fc), 0.0, np.clip(np.trunc(fc), -2147483648.0, 2147483647.0)).astype(np.int64)
    w = np.fmod(i, size)
    return np.where(w < 0, w + size, w)


def _restated(scene, w, h):
    """{layer: array} of the frame's primary hits, and the mask of the sphere pixels."""
    n = w * h
    fov_adj = math.tan(scene.fov * (math.pi / 180.0) / 2.0)  # ray.rs:45, to_radians as self * (PI / 180)
    rays = aov_ref.prime_rays(scene.fov, w, h, fov_adj)
    o = tuple(rays[:, k].copy() for k in range(3))
    d = tuple(rays[:, 3 + k].copy() for k in range(3))
    with np.errstate(divide="ignore"):
        inv = tuple(1.0 / c for c in d)             # ray.rs:23-35
    sign = tuple((c < 0.0).astype(np.int8) for c in inv)
    body = np.full(n, -1, np.int32)
    best = np.full(n, np.inf)
    for i, b in enumerate(scene.bodies):            # scene.rs:34-39: min_by keeps the first minimum
        some, t = _intersect(b, o, d, inv, sign)
        take = some & ((body < 0) | (best > t))
        body[take], best[take] = i, t[take]
    depth = np.where(body >= 0, best, np.inf)
    normal, uv = np.zeros((n, 3), F32), np.zeros((n, 2), F32)
    dc = scene.default_color
    albedo = np.tile(np.array([dc.red, dc.green, dc.blue], F32), (n, 1))
    sphere = np.zeros(n, bool)
    for i, b in enumerate(scene.bodies):
        px = np.flatnonzero(body == i)
        if not px.size:
            continue
        t = best[px]
        hit = tuple(o[k][px] + d[k][px] * t for k in range(3))  # rendering.rs:84
        if isinstance(b, Sphere):
            sphere[px] = True
            hv = _sub(hit, b.center)
            s = 1.0 / np.sqrt(_dot(hv, hv))                      # cgmath normalize: v * (1 / magnitude)
            nrm = tuple(c * s for c in hv)
            at = np.array([math.atan2(z, x) for z, x in zip(hv[2], hv[0])]).astype(F32)
            ac = np.array([math.acos(y) for y in hv[1] / b.radius]).astype(F32)
            tx, ty = (F32(1.0) + at / PI_F32) * F32(0.5), ac / PI_F32   # bodies.rs:126-132
        elif isinstance(b, (Plane, Disk)):
            nrm = tuple(np.full(px.size, -c) for c in b.normal)
            xa = _cross(b.normal, (0.0, 0.0, 1.0))               # bodies.rs:155-169, 198-212
            if _dot(xa, xa) == 0.0:
                xa = _cross(b.normal, (0.0, 1.0, 0.0))
            ya = _cross(b.normal, xa)
            hv = _sub(hit, b.origin)
            tx, ty = _dot(hv, xa).astype(F32), _dot(hv, ya).astype(F32)
        else:                                                    # bodies.rs:284-333
            lo, hi = b.bounds
            faces = [(0, lo[0], (-1.0, 0.0, 0.0)), (0, hi[0], (1.0, 0.0, 0.0)), (1, lo[1], (0.0, -1.0, 0.0)),
                     (1, hi[1], (0.0, 1.0, 0.0)), (2, lo[2], (0.0, 0.0, -1.0)), (2, hi[2], (0.0, 0.0, 1.0))]
            nv = np.zeros((px.size, 3))
            found = np.zeros(px.size, bool)
            for axis, bound, unit in faces:
                close = ~found & (np.abs(hit[axis] - bound) < 1e-8)
                nv[close] = unit
                found |= close
            assert found.all(), "the reference's AABB normal assert"
            nrm = (nv[:, 0], nv[:, 1], nv[:, 2])
            tx = ty = np.zeros(px.size, F32)
        normal[px] = np.stack(nrm, axis=1).astype(F32)
        uv[px] = np.stack([tx, ty], axis=1)
        col = b.material.coloration
        if isinstance(col, Texture):                             # material.rs:62-68
            th, tw = col.image.shape[:2]
            x, y = _wrap(tx + F32(col.x_offset), tw), _wrap(ty + F32(col.y_offset), th)
            albedo[px] = col.image[y, x, :3].astype(F32) / F32(255.0)   # color.rs:26-30
        else:
            albedo[px] = np.array([col.red, col.green, col.blue], F32)
    shape = {"body": (h, w), "depth": (h, w), "normal": (h, w, 3), "uv": (h, w, 2), "albedo": (h, w, 3)}
    out = {"body": body, "depth": depth, "normal": normal, "uv": uv, "albedo": albedo}
    return {k: v.reshape(shape[k]) for k, v in out.items()}, sphere.reshape(h, w)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_primary_hit_restated_from_the_reference(name, w, h):
    """Sphere uv goes through math.atan2 / math.acos, the libm the oracle calls: observed 0 sphere uv values
    that differ over all configs and both sizes, so every layer is compared bit for bit everywhere."""
    st, ref, _, err = _layers(name, w, h)
    assert st == 0 and err == -1
    got, sphere = _restated(config_scene(name), w, h)
    assert np.array_equal(got["body"], ref["body"]), f"{int((got['body'] != ref['body']).sum())} body ids differ"
    same = {n: aov_ref.bits(got[n]) == aov_ref.bits(ref[n]) for n in aov.LAYERS}
    for n in ("depth", "normal"):
        assert same[n].all(), f"{name} {w}x{h}: {int((~same[n]).sum())} {n} values differ"
    uv_same = same["uv"].all(axis=2)
    print(f"{name} {w}x{h}: {int((~uv_same).sum())} uv pixels differ ({int((~uv_same & sphere).sum())} on spheres)")
    assert uv_same[~sphere].all(), f"{name} {w}x{h}: uv differs off the spheres"
    if not uv_same.all():  # one f32 ulp for sphere uv only, and albedo only where uv is equal
        g, r = got["uv"][~uv_same], ref["uv"][~uv_same]
        assert (np.abs(g.astype(np.float64) - r.astype(np.float64)) <= np.spacing(np.maximum(np.abs(g), np.abs(r)))).all()
    assert same["albedo"].all(axis=2)[uv_same].all(), f"{name} {w}x{h}: albedo differs"


# ---------------------------------------------------------------- (d) the rays of the GPU module's rg_trace test
@pytest.mark.parametrize("name", ["many", "nosph"])
def test_trace_rays_are_answered_without_nan(oracle_lib, name):
    """The oracle answers mixed_scenes.trace_rays with status 0 (no RG_ERR_NAN_DISTANCE from the zero direction
    components), some rays hit and some miss, origins lie inside boxes, and the rim rays miss their disk
    although a ray a hair further in hits it unoccluded, so that `<=` in a disk test would show."""
    scene = config_scene(name)
    rays, n_rim = mixed_scenes.trace_rays(name)
    assert rays.shape == (4096, 6) and n_rim >= 1
    zero = rays[:, 3:] == 0.0
    assert (zero & ~np.signbit(rays[:, 3:])).sum() >= 256 and (zero & np.signbit(rays[:, 3:])).sum() >= 256
    boxes = [b for b in scene.bodies if isinstance(b, AABB)]
    inside = np.zeros(len(rays), bool)
    for b in boxes:
        inside |= ((rays[:, :3] > np.array(b.bounds[0])) & (rays[:, :3] < np.array(b.bounds[1]))).all(axis=1)
    assert 1000 < inside.sum() < 3000
    st, dist, body = oracle_lib.trace(SceneDesc(scene), rays)
    assert st == 0
    assert 0 < (body >= 0).sum() < len(rays) and np.isfinite(dist).all()
    rim = rays[-n_rim:]
    twin = rim.copy()
    shown = 0
    for k, r in enumerate(rim):
        disk = next(i for i, b in enumerate(scene.bodies) if isinstance(b, Disk) and b.normal == (0.0, 0.0, -1.0)
                    and abs(math.hypot(r[0] - b.origin[0], r[1] - b.origin[1]) - b.radius) < 1e-9 and r[2] > b.origin[2])
        assert body[len(rays) - n_rim + k] != disk, "a rim ray hits its disk"
        o = scene.bodies[disk].origin
        twin[k, :2] = [o[0] + (r[0] - o[0]) * (1.0 - 1e-9), o[1] + (r[1] - o[1]) * (1.0 - 1e-9)]
        shown += int(oracle_lib.trace(SceneDesc(scene), twin[k:k + 1])[2][0] == disk)
    assert shown >= 1, "every rim ray is occluded: a disk test with `<=` would not show"
