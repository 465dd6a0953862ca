"""CPU check of the host scene builder (raingun_amd/csrc/rg_scene_build.cpp): the glue between a scene
description and the tables rg_scene_create uploads -- which body goes to which table and in what order, the
values whose bits decide parity (r*r, (c.c), albedo / PI in f32, the normalised light direction), the rebased
light-buffer offsets, the rules for when a BVH, light buffers or a shadow volume are made, the statuses of a
bad description, and the LDS arena's layout and image.  tests/native/scene_build_shim.cpp puts the builder
behind a C interface; descriptions come from raingun_amd.scene.SceneDesc.  Expected values are computed here
from the description, never by a second call of the builder.  No GPU."""
import copy
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mixed_scenes import config_scene
from raingun_amd import _abi, synth
from raingun_amd.scene import SceneDesc, load_scene

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "raingun_amd" / "csrc"
GOLDEN = REPO / "tests" / "golden"
SRC = [REPO / "tests" / "native" / "scene_build_shim.cpp"] + [CSRC / f for f in (
    "rg_scene_build.cpp", "rg_bvh.cpp", "rg_lightbuf.cpp", "rg_shadow_vol.cpp")]

RG_BVH_MIN_SPHERES = 16
RG_LB_TOTAL_WORDS = 1 << 25
RG_LB_MAX_LIGHTS = 8
INVALID_ARGUMENT, TEXTURE = -1, -6

F8, F4, I4, U4 = "<f8", "<f4", "<i4", "<u4"
DTYPES = {
    "sph": [("c", F8, 3), ("r2", F8)],
    "sphf": [("c", F4, 3), ("r2hi", F4)],
    "sphf2": [("cchi", F4), ("thrp", F4), ("cc32", F4), ("id", I4)],
    "sph_cc": F8, "sph_id": I4, "pln_id": I4, "dsk_id": I4, "box_id": I4,
    "pln": [("o", F8, 3), ("n", F8, 3), ("on", F8), ("pad", F8)],
    "dsk": [("o", F8, 3), ("n", F8, 3), ("r", F8), ("on", F8)],
    "box": [("lo", F8, 3), ("hi", F8, 3)],
    "bodies": [("kind", I4), ("pad", I4), ("p", F8, 7)],
    "mats": [("coloration", I4), ("color", F4, 3), ("tex", I4), ("xoff", F4), ("yoff", F4), ("albedo_pi", F4),
             ("surface", I4), ("reflectivity", F4), ("index", F4), ("transparency", F4)],
    "lights": [("kind", I4), ("color", F4, 3), ("intensity", F4), ("pad", I4), ("v", F8, 3), ("dn", F8, 3),
               ("pad2", F8)],
    "nodes": [("raw", "u1", 128)],
    "lbuf": [("kind", I4), ("gx", I4), ("gy", I4), ("cell_off", U4), ("always0", U4), ("always1", U4),
             ("e", F4, 6), ("g0", F4, 2), ("inv", F4), ("pad", F4)],
    "lb_start": U4, "lb_ent": U4, "shvol": U4, "tex_w": U4, "tex_h": U4,
    "texs": [("texels", "<u8"), ("w", I4), ("h", I4)],
}
LAYOUT = ("sphf", "sph", "cc", "nodes", "pln", "dsk", "box", "lights", "texs", "lbuf", "bodies", "hot_bytes", "mats",
          "total_bytes", "texm", "axes", "plain_bytes", "n_sph", "n_nodes", "lbuf_staged")


class Facts(C.Structure):  # rg_scene_facts (rg_scene_tables.h)
    _fields_ = [("fov", C.c_double), ("bvh_rbound", C.c_double), ("bvh_margin", C.c_double),
                ("bvh_extent", C.c_double), ("bvh_info", _abi.rg_bvh_info),
                ("shvol_info", _abi.rg_shadow_volume_info), ("shvol_inv", C.c_float), ("shvol_off", C.c_float),
                ("bvh_obound", C.c_float), ("default_color", C.c_float * 3)] + [
        (n, C.c_int32) for n in ("n_sph", "n_pln", "n_dsk", "n_box", "n_bodies", "n_lights", "n_textures", "n_nodes",
                                 "lane_stack", "n_lbuf", "lb_cam", "n_lbdesc", "nan_scene", "pad")]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("scene_build") / "libscene_build_shim.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out),
                    *map(str, SRC)], check=True)
    lib = C.CDLL(str(out))
    lib.sb_build.restype = C.c_void_p
    lib.sb_build.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    lib.sb_free.argtypes = [C.c_void_p]
    lib.sb_table.restype = C.c_void_p
    lib.sb_table.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64)]
    lib.sb_layout_words.restype = C.c_uint32
    lib.sb_layout.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.sb_image.restype = C.c_uint64
    lib.sb_image.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_uint64]
    assert lib.sb_layout_words() == len(LAYOUT)
    return lib


class Build:
    """One rg_scene_build of a description: its tables as numpy arrays (copies), its facts."""

    def __init__(self, lib, desc):
        self.lib = lib
        st = C.c_int32(99)
        self.h = lib.sb_build(C.addressof(desc), C.byref(st))
        assert st.value == 0 and self.h
        self.raw = {k: self._bytes(k) for k in [*DTYPES, "facts"]}
        self.t = {k: np.frombuffer(self.raw[k], dtype=np.dtype(DTYPES[k])) for k in DTYPES}
        assert len(self.raw["facts"]) == C.sizeof(Facts)
        self.f = Facts.from_buffer_copy(self.raw["facts"])
        self.texels = [self._bytes(f"texels{i}") for i in range(self.f.n_textures)]

    def _bytes(self, name):
        n = C.c_uint64(0)
        p = self.lib.sb_table(self.h, name.encode(), C.byref(n))
        assert p is not None or n.value == 0
        return C.string_at(p, n.value) if n.value else b""

    def layout(self, bvh, lbuf, lstack=0):
        w = (C.c_uint32 * len(LAYOUT))()
        self.lib.sb_layout(self.h, int(bvh), int(lbuf), lstack, w)
        return dict(zip(LAYOUT, (int(v) for v in w)))

    def image(self, bvh, lbuf, lstack=0):
        n = self.lib.sb_image(self.h, int(bvh), int(lbuf), lstack, None, 0)
        buf = (C.c_uint8 * max(n, 1))()
        assert self.lib.sb_image(self.h, int(bvh), int(lbuf), lstack, buf, n) == n
        return bytes(buf)[:n]

    def close(self):
        self.lib.sb_free(self.h)
        self.h = None


def _exotic16():
    s = copy.deepcopy(synth.synthetic_scene(16))
    k = next(i for i, b in enumerate(s.bodies) if hasattr(b, "center"))
    s.bodies[k].center = (s.bodies[k].center[0], 1e100, s.bodies[k].center[2])
    return s


SCENES = {
    "test1": lambda: load_scene(GOLDEN / "examples" / "test1.yml", texture_root=GOLDEN),
    "test2": lambda: load_scene(GOLDEN / "examples" / "test2.yml", texture_root=GOLDEN),
    "test3": lambda: load_scene(GOLDEN / "examples" / "test3.yml", texture_root=GOLDEN),
    "synth15": lambda: synth.synthetic_scene(15),
    "synth16": lambda: synth.synthetic_scene(16),
    "mixed": lambda: config_scene("bvh17"),  # 17 spheres, 3 planes, 5 disks, 6 boxes, 3 lights, two textures
    "exotic16": _exotic16,
}


@pytest.fixture(scope="module")
def built(shim):
    """{name: (SceneDesc, Build)} of every scene, built once and left unchanged."""
    out = {}
    for name, make in SCENES.items():
        sd = SceneDesc(make())
        out[name] = (sd, Build(shim, sd.desc))
    yield out
    for _, b in out.values():
        b.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: "<u4", 8: "<u8"}[a.dtype.itemsize])


def _same_bits(a, b):
    return np.array_equal(_bits(np.asarray(a)), _bits(np.asarray(b, dtype=np.asarray(a).dtype)))


def _dot3(a, b):  # the reference's order: (x + y) + z, each product and sum rounded on its own
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


@pytest.mark.parametrize("name", list(SCENES))
def test_tables_follow_the_description(built, name):
    sd, b = built[name]
    d, f, t = sd.desc, b.f, b.t
    kinds = np.array([d.bodies[i].kind for i in range(d.n_bodies)], dtype=np.int64)
    p = np.array([list(d.bodies[i].p) for i in range(d.n_bodies)], dtype=np.float64).reshape(-1, 7)
    # counts
    assert (f.n_bodies, f.n_lights, f.n_textures) == (d.n_bodies, d.n_lights, d.n_textures)
    assert [f.n_sph, f.n_pln, f.n_dsk, f.n_box] == [int((kinds == k).sum()) for k in range(4)]
    assert [len(t[k]) for k in ("sph", "pln", "dsk", "box")] == [f.n_sph, f.n_pln, f.n_dsk, f.n_box]
    assert len(t["sphf"]) == len(t["sphf2"]) == f.n_sph and len(t["bodies"]) == len(t["mats"]) == d.n_bodies
    assert f.n_nodes == len(t["nodes"]) and f.n_lbdesc == len(t["lbuf"]) and f.fov == d.fov
    # the four id tables: each names bodies of its kind, together a permutation of the bodies
    ids = [t[k] for k in ("sph_id", "pln_id", "dsk_id", "box_id")]
    for k, idt in enumerate(ids):
        assert np.all(kinds[idt] == k)
    assert sorted(np.concatenate(ids).tolist()) == list(range(d.n_bodies))
    # planes, disks and boxes keep the description's order; spheres too unless a BVH reorders them
    for idt in ids[1:] + ([] if f.n_nodes else ids[:1]):
        assert np.all(np.diff(idt) > 0)
    # sphere records of table position j are those of body sph_id[j], bit for bit
    sp = p[t["sph_id"]]
    assert _same_bits(t["sph"]["c"], sp[:, :3]) and _same_bits(t["sph"]["r2"], sp[:, 3] * sp[:, 3])
    assert len(t["sph_cc"]) % 2 == 0 and len(t["sph_cc"]) - f.n_sph in (0, 1)
    assert _same_bits(t["sph_cc"][:f.n_sph], _dot3(sp, sp)) and not t["sph_cc"][f.n_sph:].any()
    assert np.array_equal(t["sphf2"]["id"], t["sph_id"])
    with np.errstate(over="ignore"):  # 1e100 rounds to +inf in f32, in the builder as here
        assert _same_bits(t["sphf"]["c"], sp[:, :3].astype(np.float32))
    # conservative f32 bounds: never below the f64 value they bound
    assert np.all(t["sphf"]["r2hi"].astype(np.float64) >= sp[:, 3] * sp[:, 3])
    assert np.all(t["sphf2"]["cchi"].astype(np.float64) >= _dot3(sp, sp))
    # the other hot tables
    pp, dp, bp = p[t["pln_id"]], p[t["dsk_id"]], p[t["box_id"]]
    assert _same_bits(t["pln"]["o"], pp[:, :3]) and _same_bits(t["pln"]["n"], pp[:, 3:6])
    assert _same_bits(t["pln"]["on"], _dot3(pp[:, :3], pp[:, 3:6]))
    assert _same_bits(t["dsk"]["o"], dp[:, :3]) and _same_bits(t["dsk"]["n"], dp[:, 3:6])
    assert _same_bits(t["dsk"]["r"], dp[:, 6]) and _same_bits(t["dsk"]["on"], _dot3(dp[:, :3], dp[:, 3:6]))
    assert _same_bits(t["box"]["lo"], bp[:, :3]) and _same_bits(t["box"]["hi"], bp[:, 3:6])
    # cold tables, in the description's order
    assert np.array_equal(t["bodies"]["kind"], kinds) and _same_bits(t["bodies"]["p"], p)
    albedo = np.array([d.bodies[i].material.albedo for i in range(d.n_bodies)], dtype=np.float32)
    assert _same_bits(t["mats"]["albedo_pi"], albedo / np.float32(3.14159265358979323846))
    assert t["mats"]["albedo_pi"].dtype == np.float32
    assert np.array_equal(t["mats"]["tex"], [d.bodies[i].material.texture for i in range(d.n_bodies)])
    assert np.array_equal(t["mats"]["surface"], [d.bodies[i].material.surface for i in range(d.n_bodies)])
    # lights: dn = normalize(-v), in the stated order of operations
    for i in range(d.n_lights):
        v = [float(c) for c in d.lights[i].v]
        n = [-c for c in v]
        inv = 1.0 / math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        assert t["lights"]["kind"][i] == d.lights[i].kind and _same_bits(t["lights"]["v"][i], v)
        assert _same_bits(t["lights"]["dn"][i], [c * inv for c in n])
    # textures
    for i in range(d.n_textures):
        w, h = d.textures[i].width, d.textures[i].height
        assert (t["tex_w"][i], t["tex_h"][i]) == (w, h)
        assert b.texels[i] == C.string_at(d.textures[i].rgba, w * h * 4)


@pytest.mark.parametrize("name", list(SCENES))
def test_rules_for_bvh_light_buffers_and_volume(built, name):
    sd, b = built[name]
    f, t = b.f, b.t
    exotic = name == "exotic16"
    assert bool(f.nan_scene) == exotic
    if f.n_sph < RG_BVH_MIN_SPHERES or exotic:
        assert f.n_nodes == 0 and f.bvh_info.built == 0 and len(t["lbuf"]) == len(t["lb_start"]) == len(t["lb_ent"]) == 0
        assert (f.n_lbuf, f.n_lbdesc, f.lb_cam, f.lane_stack) == (0, 0, -1, 0)
    else:
        assert f.n_nodes > 0 and f.bvh_info.built == 1 and f.bvh_info.nodes == f.n_nodes and 1 <= f.lane_stack <= 16
        start, ent = t["lb_start"], t["lb_ent"]
        assert len(start) + len(ent) <= RG_LB_TOTAL_WORDS
        assert f.n_lbuf in (0, min(f.n_lights, RG_LB_MAX_LIGHTS)) and f.lb_cam in (-1, f.n_lbuf if f.n_lbuf else 0)
        assert f.n_lbdesc == (f.n_lbuf if f.lb_cam < 0 else f.lb_cam + 1)
        assert f.bvh_info.lbuf_bytes == 4 * (len(start) + len(ent)) + 64 * f.n_lbdesc
        assert np.all(ent < f.n_sph)
        with_buffer = [lb for lb in t["lbuf"] if lb["kind"] != 0]
        assert with_buffer, "a 16-sphere scene whose every light and camera buffer is refused checks nothing"
        spans = []
        for lb in with_buffer:
            cells = int(lb["gx"]) * int(lb["gy"]) * (6 if lb["kind"] == 2 else 1)
            lo, hi = int(lb["cell_off"]), int(lb["cell_off"]) + cells + 1
            assert cells > 0 and hi <= len(start)
            assert np.all(np.diff(start[lo:hi].astype(np.int64)) >= 0) and start[hi - 1] <= len(ent)
            assert lb["always0"] <= lb["always1"] <= len(ent)
            spans.append((lo, hi))
        spans.sort()  # the buffers' cell starts tile lb_start without overlap
        assert spans[0][0] == 0 and spans[-1][1] == len(start)
        assert all(a[1] == c[0] for a, c in zip(spans, spans[1:]))
    if exotic or f.n_dsk or f.n_box:
        assert f.shvol_info.built == 0 and len(t["shvol"]) == 0
    if f.shvol_info.built:
        assert len(t["shvol"]) == f.shvol_info.g ** 3 and f.shvol_info.bytes == 4 * len(t["shvol"])
    assert (name in ("test1", "synth15", "synth16")) <= bool(f.shvol_info.built)


def test_bvh_threshold_sides(built):
    assert built["synth15"][1].f.n_sph == 15 and built["synth16"][1].f.n_sph == 16
    assert built["synth15"][1].f.n_nodes == 0 and built["synth16"][1].f.n_nodes > 0
    assert built["mixed"][1].f.n_dsk > 0 and built["mixed"][1].f.n_box > 0 and built["mixed"][1].f.n_nodes > 0


def _one_body_desc(**material):
    d = _abi.rg_scene_desc()
    bodies = (_abi.rg_body * 1)()
    bodies[0].kind = _abi.BODY_SPHERE
    bodies[0].p[:4] = [0.0, 0.0, -5.0, 1.0]
    bodies[0].material.texture = -1
    for k, v in material.items():
        setattr(bodies[0].material, k, v)
    lights = (_abi.rg_light * 1)()
    lights[0].v[:] = [0.0, -1.0, 0.0]
    d.fov = 90.0
    d.n_bodies, d.bodies = 1, C.cast(bodies, C.POINTER(_abi.rg_body))
    d.n_lights, d.lights = 1, C.cast(lights, C.POINTER(_abi.rg_light))
    return d, bodies, lights


def _status(lib, d):
    st = C.c_int32(99)
    h = lib.sb_build(C.addressof(d), C.byref(st))
    if h:
        lib.sb_free(h)
    return st.value


def test_statuses(shim):
    d, bodies, lights = _one_body_desc()
    assert _status(shim, d) == 0
    for field, bad in (("kind", 4), ("coloration", 2), ("surface", 3)):
        d, bodies, lights = _one_body_desc()
        if field == "kind":
            bodies[0].kind = bad
        else:
            setattr(bodies[0].material, field, bad)
        assert _status(shim, d) == INVALID_ARGUMENT, field
    d, bodies, lights = _one_body_desc()
    lights[0].kind = 2
    assert _status(shim, d) == INVALID_ARGUMENT
    # textures: index out of range (either side), zero-sized, null texels
    px = (C.c_uint8 * 16)()
    for index, w, h, rgba in ((1, 2, 2, px), (-1, 2, 2, px), (0, 0, 2, px), (0, 2, 0, px), (0, 2, 2, None)):
        d, bodies, lights = _one_body_desc(coloration=_abi.COLORATION_TEXTURE, texture=index)
        tex = (_abi.rg_texture * 1)()
        tex[0].width, tex[0].height = w, h
        if rgba is not None:
            tex[0].rgba = C.cast(rgba, C.POINTER(C.c_uint8))
        d.n_textures, d.textures = 1, C.cast(tex, C.POINTER(_abi.rg_texture))
        assert _status(shim, d) == TEXTURE, (index, w, h)
    d, bodies, lights = _one_body_desc(coloration=_abi.COLORATION_TEXTURE, texture=0)
    tex = (_abi.rg_texture * 1)()
    tex[0].width, tex[0].height, tex[0].rgba = 2, 2, C.cast(px, C.POINTER(C.c_uint8))
    d.n_textures, d.textures = 1, C.cast(tex, C.POINTER(_abi.rg_texture))
    assert _status(shim, d) == 0
    # a count without its array
    for count, array in (("n_bodies", "bodies"), ("n_lights", "lights"), ("n_textures", "textures")):
        d, bodies, lights = _one_body_desc()
        setattr(d, count, 1)
        setattr(d, array, None)
        assert _status(shim, d) == INVALID_ARGUMENT, count
    st = C.c_int32(99)
    assert shim.sb_build(None, C.byref(st)) is None and st.value == INVALID_ARGUMENT


@pytest.mark.parametrize("name", ["test1", "synth16", "mixed"])
def test_two_builds_are_identical(shim, built, name):
    sd, first = built[name]
    second = Build(shim, sd.desc)
    try:
        for k in DTYPES:
            assert first.raw[k] == second.raw[k], k
        assert first.texels == second.texels
        fa, fb = Facts.from_buffer_copy(first.raw["facts"]), Facts.from_buffer_copy(second.raw["facts"])
        fa.shvol_info.build_ms = fb.shvol_info.build_ms = 0.0  # a measurement
        assert bytes(fa) == bytes(fb)
    finally:
        second.close()


def _magic(dv):  # Granlund & Montgomery figure 4.1, as rg_exact.h packs it
    l = 0
    while l < 32 and (1 << l) < dv:
        l += 1
    return (((1 << l) - dv) << 32) // dv + 1, min(l, 1) | (max(l - 1, 0) << 8)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _plain_tables(b):
    texm = np.zeros((b.f.n_textures, 4), dtype="<u4")
    for i in range(b.f.n_textures):
        texm[i] = [*_magic(int(b.t["tex_w"][i])), *_magic(int(b.t["tex_h"][i]))]
    axes = np.zeros((b.f.n_bodies, 6), dtype="<f8")
    for i, body in enumerate(b.t["bodies"]):
        if body["kind"] == _abi.BODY_PLANE:  # bodies.rs:155-169
            n = [float(c) for c in body["p"][3:6]]
            xa = _cross(n, [0.0, 0.0, 1.0])
            if (xa[0] * xa[0] + xa[1] * xa[1]) + xa[2] * xa[2] == 0.0:
                xa = _cross(n, [0.0, 1.0, 0.0])
            axes[i] = xa + _cross(n, xa)
    return texm.tobytes(), axes.tobytes()


@pytest.mark.parametrize("lbuf", [False, True])
@pytest.mark.parametrize("bvh", [False, True])
@pytest.mark.parametrize("name", list(SCENES))
def test_arena_layout_and_image(built, name, bvh, lbuf):
    _, b = built[name]
    f, raw = b.f, b.raw
    for lstack in (0, 2 * 4 * 256 * 3):
        L = b.layout(bvh, lbuf, lstack)
        order = ["sphf", "sph", "cc", "nodes", "pln", "dsk", "box", "lights", "texs", "lbuf", "bodies", "mats",
                 "total_bytes", "axes", "plain_bytes"]
        offs = [L[k] for k in order]
        assert offs == sorted(offs) and L["sphf"] == lstack
        assert L["hot_bytes"] == L["bodies"] and L["texm"] == L["total_bytes"]
        assert L["n_sph"] == f.n_sph and L["n_nodes"] == (f.n_nodes if bvh else 0) and L["lbuf_staged"] == int(lbuf)
        # what the kernel stages in 16-byte units, and the arena's ends
        for k in order:
            assert L[k] % 16 == 0, k
        # the three runs the kernel stages up to the next member's offset: no longer than the host table
        # behind them (sph_cc is padded for this; boxes and texture descriptors are 16-byte multiples)
        for lo, hi, table in (("cc", "nodes", "sph_cc"), ("box", "lights", "box"), ("texs", "lbuf", "texs")):
            assert (L[hi] - L[lo]) % 16 == 0 and L[hi] - L[lo] <= len(raw[table]), table
    L = b.layout(bvh, lbuf)
    texm, axes = _plain_tables(b)
    segments = [("sphf", raw["sphf"] + raw["sphf2"]), ("sph", raw["sph"]), ("cc", raw["sph_cc"]),
                ("nodes", raw["nodes"] if bvh else b""), ("pln", raw["pln"]), ("dsk", raw["dsk"]), ("box", raw["box"]),
                ("lights", raw["lights"]), ("texs", raw["texs"]), ("lbuf", raw["lbuf"] if lbuf else b""),
                ("bodies", raw["bodies"]), ("mats", raw["mats"]), ("texm", texm), ("axes", axes)]
    want = bytearray(L["plain_bytes"])
    end = 0
    for k, data in segments:
        assert L[k] >= end, k  # no segment overlaps the one before it
        end = L[k] + len(data)
        want[L[k]:end] = data
    assert end <= L["plain_bytes"]
    assert b.image(bvh, lbuf) == bytes(want)
