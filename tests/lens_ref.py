"""The reference for frames through a thin lens, shared by tests/test_lens_cpu.py and tests/test_gpu_lens.py.

rgl_render of tests/native/ref_frames.c (the pinned oracle plus the camera entry's pixel loop over the sample
frame with the lens ray), through tests/ref_lib.py.  Test-side only: nothing in raingun_amd/ includes or loads it.
The tables are rg_lens_tables' (the library's host code), passed in; the resolve is raingun_amd.aa.resolve_box.
"""
import ctypes as C

import numpy as np

import ref_lib
from raingun_amd import _abi, aa
from raingun_amd.camera import Camera, Lens
from raingun_amd.scene import SceneDesc
from ref_lib import c_camera, lib

IDENTITY = Camera.identity()


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
    cc = c_camera(cam if cam is not None else IDENTITY)
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


def cached(key, scene, cam, lens, width, height, k):
    """render(), computed once per key and handed out read-only."""
    return ref_lib.cached(("lens", key, cam, lens, width, height, k), render, scene, cam, lens, width, height, k)
