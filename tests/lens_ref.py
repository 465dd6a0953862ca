"""The reference for frames through a thin lens, shared by tests/test_lens_cpu.py and tests/test_gpu_lens.py.

tests/native/lens_oracle.c (the pinned oracle plus camera_oracle.c's pixel loop over the sample frame with
the lens ray) is built into a temporary directory with the oracle's own flags, as tests/camera_ref.py
builds its file, and loaded with ctypes.  Test-side only: nothing in raingun_amd/ includes or loads it.
The tables are rg_lens_tables' (the library's host code), passed in; the resolve is raingun_amd.aa.resolve_box.
"""
import ctypes as C
import subprocess
import tempfile
from pathlib import Path

import numpy as np

import camera_ref
from raingun_amd import _abi, aa
from raingun_amd.camera import Camera, Lens
from raingun_amd.scene import SceneDesc

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "native" / "lens_oracle.c"
IDENTITY = Camera.identity()

_LIB = None
_TMP = None


def lib():
    global _LIB, _TMP
    if _LIB is None:
        _TMP = tempfile.TemporaryDirectory(prefix="lens_oracle_")
        out = Path(_TMP.name) / "liblens_oracle.so"
        cc, flags = camera_ref.oracle_flags()
        subprocess.run([cc, *flags, "-shared", "-pthread", "-o", str(out), str(SRC), "-lm"], check=True, timeout=300)
        l = C.CDLL(str(out))
        P = C.POINTER
        l.rgl_render.restype = C.c_int32
        l.rgl_render.argtypes = [P(_abi.rg_scene_desc), C.c_uint32, C.c_uint32, C.c_uint32, P(_abi.rg_camera), C.c_double,
                                 C.c_double, P(C.c_double), P(C.c_double), C.c_void_p, C.c_void_p,
                                 P(_abi.rg_ray_counts), P(C.c_int64)]
        _LIB = l
    return _LIB


def tables(k: int):
    """rg_lens_tables(k): (points (k*k, 2), rotations (64, 2)) as float64 arrays."""
    points = np.zeros((k * k, 2), np.float64)
    rotations = np.zeros((64, 2), np.float64)
    dp = C.POINTER(C.c_double)
    _abi.check(_abi.lib().rg_lens_tables(k, points.ctypes.data_as(dp), rotations.ctypes.data_as(dp)), "rg_lens_tables")
    return points, rotations


def render_samples(scene, cam, lens: Lens, width: int, height: int, k: int, points=None, rotations=None):
    """The k*height x k*width sample frame: (status, rgba, rgb, counts dict, error pixel of the SAMPLE frame)."""
    desc = scene if isinstance(scene, SceneDesc) else SceneDesc(scene)
    tp, tr = tables(k)
    points = tp if points is None else np.ascontiguousarray(points, np.float64)
    rotations = tr if rotations is None else np.ascontiguousarray(rotations, np.float64)
    assert points.shape == (k * k, 2) and rotations.shape == (64, 2)
    rgba = np.zeros((k * height, k * width, 4), dtype=np.uint8)
    rgb = np.zeros((k * height, k * width, 3), dtype=np.float32)
    counts = _abi.rg_ray_counts()
    err = C.c_int64(-1)
    cc = camera_ref.c_camera(cam if cam is not None else IDENTITY)
    dp = C.POINTER(C.c_double)
    st = lib().rgl_render(desc.ptr(), width, height, k, C.byref(cc), float(lens.aperture), float(lens.focus),
                          points.ctypes.data_as(dp), rotations.ctypes.data_as(dp), rgba.ctypes.data, rgb.ctypes.data,
                          C.byref(counts), C.byref(err))
    return st, rgba, rgb, counts.as_dict(), int(err.value)


def output_pixel(sample_pixel: int, width: int, k: int) -> int:
    """The output pixel that holds pixel `sample_pixel` of the sample frame (the AA contract's error_pixel)."""
    kw = k * width
    return (sample_pixel // kw // k) * width + (sample_pixel % kw) // k


def render(scene, cam, lens: Lens, width: int, height: int, k: int):
    """The resolved frame: (status, rgba, mean rgb, counts dict, error pixel of the OUTPUT frame or -1)."""
    st, _, rgb, counts, err = render_samples(scene, cam, lens, width, height, k)
    mean, rgba = aa.resolve_box(rgb, k)
    return st, rgba, mean, counts, (output_pixel(err, width, k) if err >= 0 else -1)


_CACHE = {}


def cached(key, scene, cam, lens, width, height, k):
    """render(), computed once per key and handed out read-only."""
    ck = (key, cam, lens, width, height, k)
    if ck not in _CACHE:
        st, rgba, mean, counts, err = render(scene, cam, lens, width, height, k)
        rgba.setflags(write=False)
        mean.setflags(write=False)
        _CACHE[ck] = (st, rgba, mean, counts, err)
    return _CACHE[ck]
