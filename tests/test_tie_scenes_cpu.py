"""The tie scenes (tests/tie_scenes.py) on the CPU, with the pinned oracle alone (no GPU needed): the conditions
that keep tests/test_gpu_ties.py from passing vacuously.

(a) Every config renders with status 0 at 97x61 and 64x40, with secondary and shadow rays.
(b) For the twinned configs the frame depends on the tie-break: rendered with the body list reversed, at least
    1000 of the 5917 pixels at 97x61 change.
(c) For the rays of the rg_trace comparison every body is traced alone, which gives each ray's distance to each
    body: at least 1000 rays have two or more bodies at the bit-equal minimum (500 of them across kinds in the
    coplanar configs), the oracle's winner is the first of them in YAML order on every ray, and on at least 500
    rays that first one is not also the last, so "keep the later one" would not go unseen.  In the coplanar
    configs the winner is, on at least 200 rays, not the tied body that the device tests first (rg_k_trace.h
    scans kind by kind), so "keep the one scanned first" would not either; twins are of one kind, and a kind's
    table keeps the YAML order unless a BVH permutes the spheres, which is (d).
(d) With a BVH, sphere ties exist whose winner's YAML id exceeds the loser's position in the sphere table, and
    others where it is below it: a leaf that hands out the table index where the YAML id is meant decides some
    ties wrongly whichever way it errs.
(e) In `coplanar` the bodies that lie in one plane win as planes, disks and boxes: the one-ulp near-ties between
    a division and a multiplication by a reciprocal go both ways.
(f) Shadow rays meet a plane, and a sphere, at exactly the light's distance (rendering.rs:152-155 is decided by
    equality there), and one ulp either side of it.
"""
import copy
import math

import numpy as np
import pytest

import tie_scenes
from raingun_amd.scene import AABB, Disk, Plane, Scene, SceneDesc, Sphere
from tie_scenes import CONFIGS, COPLANAR, TWINNED, config_scene

W, H = 97, 61
SIZES = [(97, 61), (64, 40)]
_DIST = {}


def _per_body(oracle_lib, name):
    """(bodies, rays) distances of trace_rays(name), inf where a body is missed: each body traced alone."""
    if name not in _DIST:
        scene, rays = config_scene(name), tie_scenes.trace_rays(name)
        dist = np.full((len(scene.bodies), len(rays)), np.inf)
        for i, b in enumerate(scene.bodies):
            st, d, hit = oracle_lib.trace(SceneDesc(Scene(bodies=[b])), rays)
            assert st == 0
            dist[i, hit >= 0] = d[hit >= 0]
        dist.setflags(write=False)
        _DIST[name] = dist
    return _DIST[name]


def _ties(oracle_lib, name):
    """(tied: rays with two or more bodies at the bit-equal minimum, first: the first such body per ray in YAML
    order, last: the last one, at_min: (bodies, rays) mask of the bodies at the minimum)."""
    dist = _per_body(oracle_lib, name)
    best = dist.min(axis=0)
    at_min = (dist == best[None, :]) & np.isfinite(best)[None, :]
    n_bodies = dist.shape[0]
    first = np.where(at_min.any(axis=0), at_min.argmax(axis=0), -1)
    last = np.where(at_min.any(axis=0), n_bodies - 1 - at_min[::-1].argmax(axis=0), -1)
    return at_min.sum(axis=0) >= 2, first, last, at_min


def _device_rank(scene, bvh):
    """Each body's place in the order the device scans its tables (rg_k_trace.h): spheres, planes, disks, boxes,
    each kind in YAML order; with a BVH the spheres come last (and in leaf order, which only the device knows)."""
    kind_rank = {Sphere: 3 if bvh else 0, Plane: 0 if bvh else 1, Disk: 2, AABB: 2.5}
    order = sorted(range(len(scene.bodies)), key=lambda i: (kind_rank[type(scene.bodies[i])], i))
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return rank


# ---------------------------------------------------------------- (a)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_config_renders(oracle_lib, name, w, h):
    scene = config_scene(name)
    st, rgba, _, counts, err = oracle_lib.render(SceneDesc(scene), w, h)
    assert st == 0 and err == -1
    assert counts["primary"] == w * h and counts["secondary"] > 0 and counts["shadow"] > 0
    assert len(np.unique(rgba.reshape(-1, 4), axis=0)) >= 100, "the frame shows next to nothing"


@pytest.mark.parametrize("w,h", SIZES)
def test_plain_twins_has_first_hit_tiles(w, h):
    """Some 8x8 tiles show only Diffuse winners and some do not: a PLAIN light kernel takes both of its ways
    through one frame, and in each the winner's surface, which decides the way, follows from the tie-break."""
    import aov_ref

    scene = config_scene("plain_twins")
    st, layers, _, err = aov_ref.cached(("ties", "plain_twins"), scene, w, h)
    assert st == 0 and err == -1
    voting = tie_scenes.first_hit_tiles(scene, layers["body"])
    st, layers_r, _, err = aov_ref.render(tie_scenes.reversed_bodies(scene), w, h)
    other = tie_scenes.first_hit_tiles(tie_scenes.reversed_bodies(scene), layers_r["body"])
    print(f"plain_twins {w}x{h}: {int(voting.sum())} of {voting.size} tiles are first-hit tiles, {int(other.sum())} with the body order reversed")
    assert 8 <= voting.sum() <= voting.size - 8
    assert not np.array_equal(voting, other)


def test_launch_rule_edges():
    """What tie_scenes.CONFIGS promises of the counts the launch rules look at."""
    n = {name: tie_scenes.counts(name) for name in CONFIGS}
    lights = {name: len(config_scene(name).lights) for name in CONFIGS}
    assert n["plain_twins"][2:] == (0, 0) and n["plain_twins"][0] < 16 and sum(n["plain_twins"]) < 32
    assert 1 <= lights["plain_twins"] <= 3
    assert all(k > 0 for k in n["light_twins"]) and n["light_twins"][0] < 16 and sum(n["light_twins"]) < 32
    assert n["bvh16_twins"][0] == 16 and sum(n["bvh16_twins"]) < 32 and all(k > 0 for k in n["bvh16_twins"])
    assert n["heavy_twins"][0] >= 34 and (n["heavy_twins"][0] // 2) % 2 == 1 and sum(n["heavy_twins"]) >= 32
    assert lights["heavy_twins"] == 3 and lights["heavy5l_twins"] == 5 and n["heavy5l_twins"][0] >= 16
    assert n["coplanar"][0] < 16 and sum(n["coplanar"]) < 32 and lights["coplanar"] == 3
    assert n["coplanar_bvh"][0] >= 16 and sum(n["coplanar_bvh"]) >= 32
    for name in TWINNED:  # every body has exactly one twin: the same geometry, another surface, another colour
        bodies = config_scene(name).bodies
        geo = {}
        for i, b in enumerate(bodies):
            g = copy.copy(b)
            g.material = None
            geo.setdefault(repr(g), []).append(i)
        assert all(len(v) == 2 for v in geo.values()), name
        for i, j in geo.values():
            a, b = bodies[i].material, bodies[j].material
            assert a.surface != b.surface and repr(a.coloration) != repr(b.coloration), (name, i, j)


def test_twins_keep_a_textured_pair_and_the_order():
    """At least one textured original has a twin with the other texture, and the twins of the odd-indexed
    bodies come before all the originals, those of the even-indexed ones after them, reversed."""
    from mixed_scenes import mixed_scene
    from raingun_amd.scene import Texture

    for name in TWINNED:
        base = mixed_scene(*CONFIGS[name].mixed)
        bodies = config_scene(name).bodies
        n = len(base.bodies)
        assert len(bodies) == 2 * n
        for k, b in enumerate(base.bodies):
            assert repr(bodies[n // 2 + k]) == repr(b), (name, k)
            twin = bodies[k // 2] if k % 2 else bodies[2 * n - 1 - k // 2]
            g, t = copy.copy(b), copy.copy(twin)
            g.material = t.material = None
            assert repr(g) == repr(t), (name, k)
        pairs = sum(isinstance(b.material.coloration, Texture) and isinstance(t.material.coloration, Texture)
                    and b.material.coloration.image is not t.material.coloration.image
                    for b, t in zip(base.bodies, tie_scenes.twins_of(base.bodies, CONFIGS[name].mixed[0])))
        assert pairs >= 1, f"{name}: no textured original keeps a textured twin"


def test_deterministic():
    for name in ("heavy_twins", "coplanar_bvh"):
        c = CONFIGS[name]
        from mixed_scenes import mixed_scene
        again = tie_scenes.with_twins(mixed_scene(*c.mixed), c.mixed[0]) if c.mixed else tie_scenes.coplanar_bvh_scene()
        assert again is not config_scene(name) and repr(again.bodies) == repr(config_scene(name).bodies)
    a, b = tie_scenes.trace_rays("coplanar"), tie_scenes.trace_rays("coplanar")
    assert a is b and not a.flags.writeable and a.shape == (4096, 6)
    assert (np.abs(np.sqrt((a[:, 3:] ** 2).sum(axis=1)) - 1.0) < 1e-12).all()
    assert ((a[:, :3] == 0.0).all(axis=1)).sum() == 1024, "a quarter of the rays start at the origin"


# ---------------------------------------------------------------- (b)
@pytest.mark.parametrize("name", TWINNED + ["coplanar_bvh"])
def test_frame_depends_on_the_tie_break(oracle_lib, name):
    scene = config_scene(name)
    st, fwd, _, counts, err = oracle_lib.render(SceneDesc(scene), W, H)
    st_r, rev, _, counts_r, err_r = oracle_lib.render(SceneDesc(tie_scenes.reversed_bodies(scene)), W, H)
    assert (st, err, st_r, err_r) == (0, -1, 0, -1)
    differ = int((fwd != rev).any(axis=2).sum())
    print(f"{name}: {differ} of {W * H} pixels differ between forward and reversed body order; "
          f"rays {counts} against {counts_r}")
    assert differ >= (1000 if name in TWINNED else 200)
    if name in TWINNED:
        assert counts != counts_r, "the ray counts do not depend on the tie-break"


# ---------------------------------------------------------------- (c), (d), (e)
@pytest.mark.parametrize("name", TWINNED + COPLANAR)
def test_trace_rays_tie(oracle_lib, name):
    scene, rays = config_scene(name), tie_scenes.trace_rays(name)
    tied, first, last, at_min = _ties(oracle_lib, name)
    st, dist, body = oracle_lib.trace(SceneDesc(scene), rays)
    assert st == 0 and np.isfinite(dist[body >= 0]).all()
    assert np.array_equal(body, first), "the oracle's winner is not the first minimum"
    kinds = np.array([tie_scenes.kind_of(b) for b in scene.bodies])
    n_kinds = np.array([len(set(kinds[at_min[:, r]])) for r in range(len(rays))])
    cross = int((tied & (n_kinds >= 2)).sum())
    not_last = int((tied & (first != last)).sum())
    late = {}
    for bvh in (False, True):  # the winner is not the first of the tied bodies that the device tests
        rank = _device_rank(scene, bvh)
        scanned_first = np.where(at_min, rank[:, None], len(rank)).argmin(axis=0)
        late[bvh] = int((tied & (scanned_first != first)).sum())
    print(f"{name}: {int(tied.sum())} of {len(rays)} rays tie, {cross} across kinds, the first minimum is not the "
          f"last on {not_last}, the winner is not the first one scanned on {late[False]} (linear) / {late[True]} (BVH)")
    assert tied.sum() >= 1000
    assert not_last >= 500
    if name in COPLANAR:
        assert cross >= 500
        assert late[False] >= 200 and late[True] >= 200
    assert 0 < (body >= 0).sum()


@pytest.mark.parametrize("name", ["bvh16_twins", "heavy_twins", "heavy5l_twins", "coplanar_bvh"])
def test_sphere_ties_against_the_table_order(oracle_lib, name):
    """From the descriptor order (what rg_scene_create groups by kind): position of each sphere in the sphere
    table, against the YAML ids.  Spheres tie where both are at the minimum."""
    scene = config_scene(name)
    desc = SceneDesc(scene)
    from raingun_amd import _abi
    is_sph = [desc.desc.bodies[i].kind == _abi.BODY_SPHERE for i in range(desc.desc.n_bodies)]
    assert is_sph == [isinstance(b, Sphere) for b in scene.bodies] and sum(is_sph) >= 16
    table_pos = np.cumsum(is_sph) - 1
    tied, first, _, at_min = _ties(oracle_lib, name)
    above = below = 0
    for r in np.flatnonzero(tied):
        w = first[r]
        if not is_sph[w]:
            continue
        for l in np.flatnonzero(at_min[:, r]):
            if l != w and is_sph[l]:
                above += int(w > table_pos[l])
                below += int(w < table_pos[l])
    print(f"{name}: sphere ties whose winner's YAML id is above the loser's table position: {above}, below: {below}")
    assert above >= 1 and below >= 1


def test_coplanar_near_ties_go_both_ways(oracle_lib):
    """Among the rays whose winner lies in the floor (or in the back wall), planes, disks and boxes all win."""
    scene = config_scene("coplanar")
    _, _, body = oracle_lib.trace(SceneDesc(scene), tie_scenes.trace_rays("coplanar"))
    for plane_bodies in (tie_scenes.COPLANAR_FLOOR, tie_scenes.COPLANAR_WALL):
        wins = {type(scene.bodies[i]).__name__: int((body == i).sum()) for i in plane_bodies}
        by_kind = {}
        for i in plane_bodies:
            k = type(scene.bodies[i]).__name__
            by_kind[k] = by_kind.get(k, 0) + int((body == i).sum())
        print(f"coplanar, bodies {plane_bodies}: winners {by_kind}")
        assert sum(n >= 20 for n in by_kind.values()) >= 2, wins
    # the second floor plane wins nowhere: its distance is the first one's to the bit (|n| = 4 scales exactly)
    assert (body == 3).sum() == 0 and (body == 1).sum() > 0
    # and the construction is what the docstring says
    b = scene.bodies
    assert isinstance(b[1], Plane) and isinstance(b[3], Plane) and isinstance(b[2], AABB) and isinstance(b[0], Disk)
    assert b[2].bounds[1][1] == b[1].origin[1] == b[3].origin[1] == b[0].origin[1] == b[4].origin[1] == b[16].origin[1]
    assert b[7].bounds[1][2] == b[6].origin[2] == b[5].origin[2] == b[8].origin[2]
    assert b[9].center[1] - b[9].radius == tie_scenes.FLOOR_Y
    assert math.dist(b[10].center, b[11].center) == b[10].radius + b[11].radius
    assert b[12].center == b[13].center and b[12].material.surface == "Refractive"
    assert b[14].bounds[1][2] == b[15].bounds[1][2]
    inner = b[15].bounds
    assert all(l < p < h for l, p, h in zip(inner[0], scene.lights[0].position, inner[1]))


# ---------------------------------------------------------------- (f)
def test_shadow_rays_end_at_the_lights_own_distance(oracle_lib):
    """Shadow rays towards the light in the back wall, from points in front of it: the wall's distance, as
    bodies.rs:137-148 computes it, equals the light's (lights.rs:53-58) on many rays, and lies one ulp either
    side of it on others; the same for the light on a sphere's surface, from the side it is on."""
    rng = np.random.default_rng(5)
    n = 4096
    for light, body, where in ((tie_scenes.LIGHT_IN_WALL, config_scene("coplanar").bodies[6], "wall"),
                               (tie_scenes.LIGHT_ON_SPHERE, Sphere(*tie_scenes.LIT_SPHERE, None), "sphere")):
        o = np.stack([rng.uniform(-9.0, 6.0, n), rng.uniform(-3.0, 6.0, n), rng.uniform(-30.0, -5.0, n)], axis=1)
        v = np.array(light)[None, :] - o
        ld = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])   # cgmath magnitude
        d = v * (1.0 / ld)[:, None]                                                   # normalize: v * (1 / magnitude)
        b = copy.copy(body)
        b.material = config_scene("coplanar").bodies[1].material
        st, t, hit = oracle_lib.trace(SceneDesc(Scene(bodies=[b])), np.concatenate([o, d], axis=1))
        assert st == 0
        hit = hit >= 0
        near = hit & (np.abs(t - ld) <= 4 * np.spacing(ld))
        equal, below, above = (int((near & c).sum()) for c in (t == ld, t < ld, t > ld))
        print(f"{where}: of {n} shadow rays {int(near.sum())} end at the light: t == ld {equal}, t < ld {below}, t > ld {above}")
        assert equal >= 100 and above >= 100
