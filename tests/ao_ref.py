"""The reference for the ambient occlusion pass, shared by tests/test_ao_cpu.py and tests/test_gpu_ao.py.

rgao_render of tests/native/ao_ref.c: tests/native/ref_frames.c unchanged (the pinned oracle, the pixel loop, the
camera ray) plus one entry that traces the primary ray as rga_render does and then, with the oracle's
surface_normal and trace, the k x k rays of include/raingun.h's contract.  Built once per session as
tests/ref_lib.py builds its library (the oracle's own compiler and flags) and loaded with ctypes.  Test-side
only: nothing in raingun_amd/ includes or loads it.  The tables are rg_ao_tables' / rg_lens_tables' (the
library's host code), passed in.
"""
import ctypes as C
import subprocess
import tempfile
from pathlib import Path

import numpy as np

import ref_lib
from raingun_amd import _abi, ao
from raingun_amd.scene import SceneDesc
from ref_lib import c_camera

SRC = ref_lib.REPO / "tests" / "native" / "ao_ref.c"

_LIB = None
_TMP = None


def lib():
    global _LIB, _TMP
    if _LIB is None:
        _TMP = tempfile.TemporaryDirectory(prefix="ao_ref_")
        out = Path(_TMP.name) / "libao_ref.so"
        cc, flags = ref_lib.oracle_flags()
        subprocess.run([cc, *flags, "-shared", "-pthread", "-o", str(out), str(SRC), "-lm"], check=True, timeout=300)
        l = C.CDLL(str(out))
        P = C.POINTER
        dp = P(C.c_double)
        l.rgao_render.restype = C.c_int32
        l.rgao_render.argtypes = [P(_abi.rg_scene_desc), C.c_uint32, C.c_uint32, P(_abi.rg_tiling), P(_abi.rg_camera),
                                  C.c_uint32, C.c_double, C.c_double, dp, dp, C.c_void_p, C.c_void_p, C.c_void_p,
                                  P(_abi.rg_ray_counts), P(C.c_int64)]
        l.rgo_tiling_rows.restype = C.c_uint32
        l.rgo_tiling_rows.argtypes = [C.c_uint32, P(_abi.rg_tiling)]
        _LIB = l
    return _LIB


def render(scene, width: int, height: int, samples: int, radius: float = float("inf"), bias: float = 1e-13, cam=None,
           tile_rows: int = 0, stride: int = 1, offset: int = 0, want_rays: bool = False):
    """The reference's frame: (status, ao (rows, W) float32, counts dict, error_pixel, open (rows, W) int32 -- -1 on
    a miss --, rays (rows, W, k*k, 6) float64 or None)."""
    desc = scene if isinstance(scene, SceneDesc) else SceneDesc(scene)
    t = _abi.rg_tiling(tile_rows or height, stride, offset)
    rows = lib().rgo_tiling_rows(height, C.byref(t))
    k2 = samples * samples
    out = np.zeros((rows, width), np.float32)
    opened = np.zeros((rows, width), np.int32)
    rays = np.zeros((rows, width, k2, 6), np.float64) if want_rays else None
    points, turns = ao.tables(samples), ao.rotations()
    counts = _abi.rg_ray_counts()
    err = C.c_int64(-1)
    cc = c_camera(cam) if cam is not None else None
    dp = C.POINTER(C.c_double)
    st = lib().rgao_render(desc.ptr(), width, height, C.byref(t), C.byref(cc) if cc is not None else None, samples,
                           radius, bias, points.ctypes.data_as(dp), turns.ctypes.data_as(dp), out.ctypes.data,
                           opened.ctypes.data, rays.ctypes.data if rays is not None else None, C.byref(counts),
                           C.byref(err))
    return st, out, counts.as_dict(), int(err.value), opened, rays


def cached(key, scene, width, height, samples, radius=float("inf"), bias=1e-13, cam=None, **tiling):
    """render() without the rays, computed once per key and handed out read-only."""
    k = ("ao", key, cam, width, height, samples, float(radius), float(bias), tuple(sorted(tiling.items())))
    return ref_lib.cached(k, render, scene, width, height, samples, radius, bias, cam, **tiling)
