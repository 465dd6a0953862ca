"""The reference for frames with area lights, shared by tests/test_area_cpu.py and tests/test_gpu_area.py.

rgar_render of tests/native/area_ref.c: tests/native/ref_frames.c unchanged (the pinned oracle, the pixel loop, the
camera ray and the lens ray) plus one entry that, per sample, moves the spherical lights in a copy of the light
array and calls the existing colour path.  Built once per session as tests/ref_lib.py builds its library (the
oracle's own compiler and flags) and loaded with ctypes.  Test-side only: nothing in raingun_amd/ includes or
loads it.  The tables are rg_area_tables' / rg_lens_tables' (the library's host code); the resolve is
raingun_amd.aa.resolve_box.
"""
import ctypes as C
import subprocess
import tempfile
from pathlib import Path

import numpy as np

import lens_ref
import ref_lib
from raingun_amd import _abi, aa
from raingun_amd.camera import Camera
from raingun_amd.scene import SceneDesc
from ref_lib import c_camera

SRC = ref_lib.REPO / "tests" / "native" / "area_ref.c"
IDENTITY = Camera.identity()

_LIB = None
_TMP = None


def lib():
    global _LIB, _TMP
    if _LIB is None:
        _TMP = tempfile.TemporaryDirectory(prefix="area_ref_")
        out = Path(_TMP.name) / "libarea_ref.so"
        cc, flags = ref_lib.oracle_flags()
        subprocess.run([cc, *flags, "-shared", "-pthread", "-o", str(out), str(SRC), "-lm"], check=True, timeout=300)
        l = C.CDLL(str(out))
        P = C.POINTER
        dp = P(C.c_double)
        l.rgar_render.restype = C.c_int32
        l.rgar_render.argtypes = [P(_abi.rg_scene_desc), C.c_uint32, C.c_uint32, C.c_uint32, P(_abi.rg_camera), C.c_double,
                                  C.c_double, dp, dp, dp, dp, C.c_void_p, C.c_void_p, P(_abi.rg_ray_counts), P(C.c_int64)]
        _LIB = l
    return _LIB


def tables(k: int):
    """rg_area_tables(k): the points (k*k, 3) as a float64 array."""
    points = np.zeros((k * k, 3), np.float64)
    _abi.check(_abi.lib().rg_area_tables(k, points.ctypes.data_as(C.POINTER(C.c_double))), "rg_area_tables")
    return points


def render_samples(scene, cam, lens, radii, width: int, height: int, k: int):
    """The k*height x k*width sample frame: (status, rgba, rgb, counts dict, error pixel of the SAMPLE frame).
    lens: a Lens or None (the camera ray); radii: one per light."""
    desc = scene if isinstance(scene, SceneDesc) else SceneDesc(scene)
    lens_points, rotations = lens_ref.tables(k)
    sphere_points = tables(k)
    radii = np.ascontiguousarray(radii, np.float64)
    assert radii.shape == (desc.desc.n_lights,), (radii.shape, desc.desc.n_lights)
    rgba = np.zeros((k * height, k * width, 4), dtype=np.uint8)
    rgb = np.zeros((k * height, k * width, 3), dtype=np.float32)
    counts = _abi.rg_ray_counts()
    err = C.c_int64(-1)
    cc = c_camera(cam if cam is not None else IDENTITY)
    dp = C.POINTER(C.c_double)
    aperture, focus = (float(lens.aperture), float(lens.focus)) if lens is not None else (0.0, 1.0)
    pad = np.zeros(1)  # a scene without lights: a pointer all the same
    st = lib().rgar_render(desc.ptr(), width, height, k, C.byref(cc), aperture, focus, lens_points.ctypes.data_as(dp),
                           rotations.ctypes.data_as(dp), sphere_points.ctypes.data_as(dp),
                           (radii if radii.size else pad).ctypes.data_as(dp), rgba.ctypes.data, rgb.ctypes.data,
                           C.byref(counts), C.byref(err))
    return st, rgba, rgb, counts.as_dict(), int(err.value)


def render(scene, cam, lens, radii, width: int, height: int, k: int):
    """The resolved frame: (status, rgba, mean rgb, counts dict, error pixel of the OUTPUT frame or -1)."""
    st, _, rgb, counts, err = render_samples(scene, cam, lens, radii, width, height, k)
    mean, rgba = aa.resolve_box(rgb, k)
    return st, rgba, mean, counts, (lens_ref.output_pixel(err, width, k) if err >= 0 else -1)


def cached(key, scene, cam, lens, radii, width, height, k):
    """render(), computed once per key and handed out read-only."""
    return ref_lib.cached(("area", key, cam, lens, tuple(float(r) for r in radii), width, height, k), render, scene, cam,
                          lens, radii, width, height, k)
