"""CPU check of the PLAIN light kernels' shadow mask volume (raingun_amd/csrc/rg_shadow_vol.cpp +
the kernel's cell lookup rg_shadow_vol_cell.h): tests/native/shadow_vol_sim.cpp casts shadow rays
towards every light from sphere surfaces (with the shadow bias), from points on the planes, from
random points in and around the domain (outside it: the all-ones word), grazing rays that pass at
r (1 +- 1e-9) and r (1 +- 1e-13) from a sphere's centre, and rays from cell faces and corners, and
requires of every ray and body: if the exact reference test accepts the body, its bit is set in the
ray's cell.  A negative control shrinks the footprints by 1 % and drops the margins, and must be
caught.  The admission predicate is checked on the scenes it must refuse."""
import json
import math
import subprocess
from pathlib import Path

import pytest

from raingun_amd import synth
from raingun_amd._host import LoadedScene

REPO = Path(__file__).resolve().parent.parent
SRC = [REPO / "tests" / "native" / "shadow_vol_sim.cpp", REPO / "raingun_amd" / "csrc" / "rg_shadow_vol.cpp"]
G = 64  # RG_SHVOL_G


def _build(tmp_path_factory, extra=()):
    out = tmp_path_factory.mktemp("sv") / "shadow_vol_sim"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", str(out), *map(str, SRC)], check=True)
    return out


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return _build(tmp_path_factory)


def _text(spheres, planes, lights):
    """spheres (cx, cy, cz, r), planes (ox, oy, oz, nx, ny, nz), lights (kind, (x, y, z))."""
    num = lambda vs: " ".join(repr(float(v)) for v in vs)
    lines = [str(len(spheres))] + [num(s) for s in spheres] + [str(len(planes))] + [num(p) for p in planes]
    lines += [str(len(lights))] + [f"{k} {num(v)}" for k, v in lights]
    return "\n".join(lines) + "\n"


def _desc_tables(d):
    sp = [tuple(d.bodies[i].p[:4]) for i in range(d.n_bodies) if d.bodies[i].kind == 0]
    pl = [tuple(d.bodies[i].p[:6]) for i in range(d.n_bodies) if d.bodies[i].kind == 1]
    lights = [(d.lights[i].kind, tuple(d.lights[i].v)) for i in range(d.n_lights)]
    return sp, pl, lights


def _run(exe, text, rays=2000, g=G, fov=None):
    args = [str(exe), str(rays), str(g)] + ([repr(float(fov))] if fov else [])
    r = subprocess.run(args, input=text, capture_output=True, text=True, timeout=600)
    return r.returncode, (json.loads(r.stdout) if r.stdout.strip() else None), r.stderr


def _test1_tables(example_scenes):
    from raingun_amd.scene import SceneDesc

    return _desc_tables(SceneDesc(example_scenes["test1"]).desc)


def test_test1(sim, example_scenes):
    """test1's bodies and lights; the program also prints the share of set bits and the kept
    fractions per 8x8 tile of the primary hits at 960x536 (nothing is asserted about those)."""
    sp, pl, lights = _test1_tables(example_scenes)
    assert (len(sp), len(pl), len(lights)) == (4, 2, 3)
    rc, res, err = _run(sim, _text(sp, pl, lights), rays=3000, fov=example_scenes["test1"].fov)
    print(json.dumps(res))
    assert rc == 0, err
    assert res["violations"] == 0 and res["accepted"] > 5000 and res["grazing"] > 5000
    assert res["no_cell"] > 1000 and res["lattice_points"] > 3000


def test_synthetic_16(sim):
    ls = LoadedScene.from_string(synth.synthetic_yaml(16))
    sp, pl, lights = _desc_tables(ls.desc)
    ls.close()
    assert len(sp) == 16 and len(pl) == 2
    rc, res, err = _run(sim, _text(sp[:16], pl, lights))
    assert rc == 0, err
    assert res["violations"] == 0 and res["accepted"] > 5000 and res["grazing"] > 3000


def test_one_sphere_with_a_light_inside_and_one_on_its_surface(sim):
    sp = [(0.5, 1.0, -10.0, 2.0)]
    lights = [(1, (0.8, 1.2, -10.5)), (1, (0.5, 3.0, -10.0)), (0, (0.3, -1.0, -0.2))]
    rc, res, err = _run(sim, _text(sp, [], lights), rays=6000)
    assert rc == 0, err
    assert res["violations"] == 0 and res["accepted"] > 5000


def _ulps(x, n):
    for _ in range(abs(n)):
        x = math.nextafter(x, math.inf if n > 0 else -math.inf)
    return x


def test_planes_only(sim):
    """Planes only: normals whose den against the directional light lies within a few ulps of the
    test's 1e-6 on both sides, and spherical lights 3 ulps off the floor plane on either side."""
    dirv = (0.4, -1.0, -0.9)
    n = math.sqrt(sum(c * c for c in dirv))
    dn = tuple(-c / n for c in dirv)
    # a unit vector t perpendicular to dn: normals t + c dn have den = c (1 + rounding)
    t = (dn[1], -dn[0], 0.0)
    tn = math.sqrt(sum(c * c for c in t))
    t = tuple(c / tn for c in t)
    planes = [(0.0, -2.0, 0.0, 0.0, -1.0, 0.0), (0.0, 0.0, -40.0, 0.0, 0.0, -1.0), (0.0, 30.0, 0.0, 0.0, 1.0, 0.0)]
    inv = 1.0 / math.sqrt((dirv[0] * dirv[0] + dirv[1] * dirv[1]) + dirv[2] * dirv[2])
    dnk = tuple(-c * inv for c in dirv)  # RgLightDev::dn, as rg_scene.hip rounds it
    den = lambda nv: (nv[0] * dnk[0] + nv[1] * dnk[1]) + nv[2] * dnk[2]  # the kernel's expression
    for k in (-3, -1, 0, 1, 2, 4):
        want = _ulps(1e-6, k)
        nv = [t[0] + 1e-6 * dn[0], t[1] + 1e-6 * dn[1], 0.0]
        nv[2] = (want - den(nv)) / dnk[2]  # t has no z: the last term tunes den an ulp of nv[2] at a time
        for _ in range(256):
            if den(nv) == want:
                break
            nv[2] = _ulps(nv[2], 1 if den(nv) < want else -1)
        assert abs(den(nv) - 1e-6) < 1e-6 * 2e-15, (k, den(nv))
        planes.append((5.0, 1.0, -20.0) + tuple(nv))
    lights = [(0, dirv), (1, (3.0, _ulps(-2.0, 3), -7.0)), (1, (-4.0, _ulps(-2.0, -3), -9.0))]
    rc, res, err = _run(sim, _text([], planes, lights), rays=20000)
    assert rc == 0, err
    assert res["violations"] == 0 and res["accepted"] > 5000
    assert res["den_near_1e-6"] >= 3


def _corner_scene(g=G):
    """A cell, a light far along u from its centre b and a sphere at 0.995 (r + rho) from b along a
    cube diagonal perpendicular to u: the cell's corner towards the sphere lies inside it, so the
    exact test accepts the sphere from there, with the segment [b, L] almost r + rho away."""
    far = (0.0, 0.0, -50.0, 1.0)  # fixes S = 51, O = 205
    O = 4.0 * 51.0 + 1.0
    e = 2.0 * O / g
    rho = e * math.sqrt(3.0) / 2.0
    b = tuple(-O + (i + 0.5) * e for i in (g // 2 + 2, g // 2 + 2, g // 2 - 2))
    w = tuple(1.0 / math.sqrt(3.0) for _ in range(3))
    u = (1.0 / math.sqrt(2.0), -1.0 / math.sqrt(2.0), 0.0)
    r = 1.0
    c = tuple(b[i] + w[i] * (r + rho) * 0.995 for i in range(3))
    L = tuple(b[i] + 1000.0 * u[i] for i in range(3))
    return _text([far, c + (r,)], [], [(1, L)])


def test_corner_scene(sim):
    rc, res, err = _run(sim, _corner_scene())
    assert rc == 0, err
    assert res["violations"] == 0 and res["accepted"] > 1000


def test_dropped_margins_are_caught(tmp_path_factory):
    exe = _build(tmp_path_factory, ["-DRG_SHVOL_TEST_NO_MARGIN"])
    rc, res, _ = _run(exe, _corner_scene())
    assert rc == 1 and res["violations"] > 0


def _grid(n, kind):
    if kind == "sphere":
        return [(3.0 * (i % 5), 3.0 * (i // 5), -10.0, 1.0) for i in range(n)]
    return [(0.0, 0.0, -50.0 - i, 0.0, 0.0, -1.0) for i in range(n)]


LIGHT = [(1, (5.0, 20.0, -5.0))]


@pytest.mark.parametrize("name,text,admitted", [
    ("16 spheres", _text(_grid(16, "sphere"), [], LIGHT), True),
    ("17 spheres", _text(_grid(17, "sphere"), [], LIGHT), False),
    ("16 planes", _text([], _grid(16, "plane"), LIGHT), True),
    ("17 planes", _text([], _grid(17, "plane"), LIGHT), False),
    ("non-finite light", _text(_grid(2, "sphere"), [], [(1, (5.0, float("inf"), -5.0))]), False),
    ("NaN light", _text(_grid(2, "sphere"), [], [(1, (float("nan"), 1.0, -5.0))]), False),
    ("zero bodies", _text([], [], LIGHT), False),
    ("four lights", _text(_grid(2, "sphere"), [], LIGHT * 4), False),
    ("no light", _text(_grid(2, "sphere"), [], []), False),
    ("magnitude", _text([(0.0, 0.0, -2.0e6, 1.0)], [], LIGHT), False),
])
def test_admission(sim, name, text, admitted):
    rc, res, err = _run(sim, text, rays=50)
    assert res["admitted"] == (1 if admitted else 0), name
    assert rc == (0 if admitted else 3), err
