"""The reference for the ambient term, shared by tests/test_ambient_cpu.py and tests/test_gpu_ambient.py.

tests/native/ambient_ref.c: the edge-stopping filter, the per-body share and the compose in plain C, written from
the header's text, built once per session with the oracle's own compiler and flags (as tests/ao_ref.py builds its
library) and loaded with ctypes.  frame() puts a whole ambient frame together from the references of its passes:
the supersampled beauty frame (tests/area_ref.py, which knows the camera, the lens and the light radii), the AOV
layers (tests/aov_ref.py) and the AO pass (tests/ao_ref.py).  Test-side only: nothing in raingun_amd/ includes or
loads it.
"""
import ctypes as C
import subprocess
import tempfile
from pathlib import Path

import numpy as np

import ao_ref
import aov_ref
import area_ref
import ref_lib
from raingun_amd import _abi
from raingun_amd.scene import SceneDesc

SRC = ref_lib.REPO / "tests" / "native" / "ambient_ref.c"
PANICS = (_abi.RG_ERR_AABB_NORMAL, _abi.RG_ERR_NAN_DISTANCE, _abi.RG_ERR_TRANSMISSION)

_LIB = None
_TMP = None


def lib():
    global _LIB, _TMP
    if _LIB is None:
        _TMP = tempfile.TemporaryDirectory(prefix="ambient_ref_")
        out = Path(_TMP.name) / "libambient_ref.so"
        cc, flags = ref_lib.oracle_flags()
        subprocess.run([cc, *flags, "-shared", "-o", str(out), str(SRC), "-lm"], check=True, timeout=300)
        l = C.CDLL(str(out))
        V, U32 = C.c_void_p, C.c_uint32
        l.amb_filter.restype = l.amb_pairs.restype = l.amb_shares.restype = l.amb_compose.restype = None
        l.amb_filter.argtypes = [V, V, V, U32, U32, U32, C.c_float, C.c_int32, V]
        l.amb_pairs.argtypes = [V, V, U32, U32, U32, C.c_float, C.POINTER(C.c_uint64), V]
        l.amb_shares.argtypes = [C.POINTER(_abi.rg_scene_desc), V]
        l.amb_compose.argtypes = [V, V, V, V, V, C.POINTER(C.c_float), C.c_uint64, V, V]
        _LIB = l
    return _LIB


def _layers(ao, body, normal):
    a = np.ascontiguousarray(ao, np.float32)
    b = np.ascontiguousarray(body, np.int32)
    n = np.ascontiguousarray(normal, np.float32)
    assert a.ndim == 2 and b.shape == a.shape and n.shape == (*a.shape, 3), (a.shape, b.shape, n.shape)
    return a, b, n


def filter_ao(ao, body, normal, radius, normal_min, reverse=False):
    """(H, W) float32: the reference's filter; reverse: the taps backwards (not the contract)."""
    a, b, n = _layers(ao, body, normal)
    h, w = a.shape
    out = np.zeros((h, w), np.float32)
    lib().amb_filter(a.ctypes.data, b.ctypes.data, n.ctypes.data, w, h, int(radius), float(normal_min), int(bool(reverse)),
                     out.ctypes.data)
    return out


def pairs(body, normal, radius, normal_min):
    """(in-frame pairs of a hit pixel and another pixel of its window, accepted ones among them, (H, W) bool: the hit
    pixels with an in-frame neighbour the filter rejects)."""
    b = np.ascontiguousarray(body, np.int32)
    n = np.ascontiguousarray(normal, np.float32)
    h, w = b.shape
    count = (C.c_uint64 * 2)()
    rejecting = np.zeros((h, w), np.uint8)
    lib().amb_pairs(b.ctypes.data, n.ctypes.data, w, h, int(radius), float(normal_min), count, rejecting.ctypes.data)
    return int(count[0]), int(count[1]), rejecting.astype(bool)


def shares(scene):
    desc = scene if isinstance(scene, SceneDesc) else SceneDesc(scene)
    out = np.zeros(max(int(desc.desc.n_bodies), 1), np.float32)
    lib().amb_shares(desc.ptr(), out.ctypes.data)
    return out[:int(desc.desc.n_bodies)]


def compose(rgb, albedo, body, aof, share, color):
    """((H, W, 3) float32 clamped colours, (H, W, 4) uint8 frame)."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    albedo = np.ascontiguousarray(albedo, np.float32)
    body = np.ascontiguousarray(body, np.int32)
    aof = np.ascontiguousarray(aof, np.float32)
    share = np.ascontiguousarray(np.concatenate([np.asarray(share, np.float32).reshape(-1), np.zeros(1, np.float32)]))
    col = (C.c_float * 3)(*[float(c) for c in np.broadcast_to(np.asarray(color, np.float32).reshape(-1), (3,))])
    out = np.zeros(rgb.shape, np.float32)
    rgba = np.zeros((*body.shape, 4), np.uint8)
    lib().amb_compose(rgb.ctypes.data, albedo.ctypes.data, body.ctypes.data, aof.ctypes.data, share.ctypes.data, col,
                      body.size, out.ctypes.data, rgba.ctypes.data)
    return out, rgba


def frame(key, scene, width, height, color, samples, ao_spec, filter_radius, normal_min, cam=None, lens=None, radii=None):
    """A whole ambient frame on the reference: a dict with status, error_pixel, counts, rgba, rgb (the clamped
    colours), aof (the filtered pass, or the raw one at filter_radius 0), raw, body, normal, albedo, beauty_rgba."""
    desc = scene if isinstance(scene, SceneDesc) else SceneDesc(scene)
    k, radius, bias = ao_spec
    rr = np.zeros(int(desc.desc.n_lights)) if radii is None else np.asarray(radii, np.float64)
    b_st, b_rgba, b_rgb, b_counts, b_err = area_ref.cached(key, scene, cam, lens, rr, width, height, samples)
    l_st, layers, l_counts, l_err = aov_ref.cached(key, scene, width, height, cam)
    a_st, raw, a_counts, a_err, _, _ = ao_ref.cached(key, scene, width, height, k, radius, bias, cam)
    for st in (b_st, l_st, a_st):
        assert st == 0 or st in PANICS, st
    aof = filter_ao(raw, layers["body"], layers["normal"], filter_radius, normal_min) if filter_radius else raw
    rgb, rgba = compose(b_rgb, layers["albedo"], layers["body"], aof, shares(desc), color)
    status, err = 0, -1
    for st, e in ((b_st, b_err), (l_st, l_err), (a_st, a_err)):  # the lowest failing pixel; a tie keeps the earlier pass
        if st != 0 and (status == 0 or e < err):
            status, err = st, e
    counts = {c: b_counts[c] + l_counts[c] + a_counts[c] for c in b_counts}
    return {"status": status, "error_pixel": err, "counts": counts, "rgba": rgba, "rgb": rgb, "aof": aof, "raw": raw,
            "body": layers["body"], "normal": layers["normal"], "albedo": layers["albedo"], "beauty_rgba": b_rgba}
