"""CPU count of the tiles that pass the vote of the PLAIN light kernels' first-hit path
(raingun_amd/csrc/rg_render_kernel.h): tests/native/first_hit_tiles_sim.cpp traces the
primary rays of a frame and counts the 8x8 tiles whose pixels all end at a miss, a Diffuse body, or a
Reflecting body with max_depth <= 1.  The share of such tiles is what the path can be worth; the counts
at the GPU tests' frame sizes are what tests/test_gpu_first_hit_tile.py expects of the kernels."""
import json
import subprocess
from pathlib import Path

import pytest

from raingun_amd import _abi
from raingun_amd.scene import SceneDesc

REPO = Path(__file__).resolve().parent.parent
SRC = REPO / "tests" / "native" / "first_hit_tiles_sim.cpp"


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = tmp_path_factory.mktemp("fh") / "first_hit_tiles_sim"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(out), str(SRC)], check=True)
    return out


def _text(scene):
    """The scene's spheres and planes with their surface class, in the program's format."""
    owner = SceneDesc(scene)  # owns the arrays d points into
    d = owner.desc
    num = lambda vs: " ".join(repr(float(v)) for v in vs)
    rows = {_abi.BODY_SPHERE: [], _abi.BODY_PLANE: []}
    for i in range(d.n_bodies):
        b = d.bodies[i]
        rows[b.kind].append(f"{num(b.p[:4 if b.kind == _abi.BODY_SPHERE else 6])} {b.material.surface}")
    sp, pl = rows[_abi.BODY_SPHERE], rows[_abi.BODY_PLANE]
    assert len(sp) + len(pl) == d.n_bodies, "spheres and planes only"
    return "\n".join([str(len(sp)), *sp, str(len(pl)), *pl]) + "\n"


def _run(exe, scene, w, h, depth=None):
    depth = scene.max_recursion_depth if depth is None else depth
    r = subprocess.run([str(exe), str(w), str(h), repr(float(scene.fov)), str(depth)], input=_text(scene),
                       capture_output=True, text=True, timeout=300, check=True)
    res = json.loads(r.stdout)
    assert sum(res["rows"]) == res["voting"] and res["tiles"] == ((w + 7) // 8) * ((h + 7) // 8)
    return res


def test_test1_share(sim, example_scenes):
    """Nine tiles in ten of test1 need no recursion state (counted when the path was proposed: 0.8953)."""
    res = _run(sim, example_scenes["test1"], 960, 536)
    share = res["voting"] / res["tiles"]
    print(json.dumps({"tiles": res["tiles"], "voting": res["voting"], "share": round(share, 4)}))
    assert res["tiles"] == 120 * 67
    assert share >= 0.85


@pytest.mark.parametrize("w,h,voting,tiles", [(97, 61, 83, 104), (64, 40, 30, 40)])
def test_test1_at_the_gpu_tests_sizes(sim, example_scenes, w, h, voting, tiles):
    res = _run(sim, example_scenes["test1"], w, h)
    assert (res["voting"], res["tiles"]) == (voting, tiles)


def test_depth_one_admits_the_reflecting_bodies(sim, example_scenes):
    """With max_depth 1 a Reflecting hit mixes with the default colour and pushes no frame: more tiles vote."""
    deep = _run(sim, example_scenes["test1"], 97, 61)
    one = _run(sim, example_scenes["test1"], 97, 61, depth=1)
    assert deep["voting"] < one["voting"] < one["tiles"]  # the refractive sphere stays outside
