"""The reference for AOV layers, shared by tests/test_aov_cpu.py and tests/test_gpu_aov.py.

rga_render of tests/native/ref_frames.c (the pinned oracle plus its pixel loop stopping after the primary hit),
through tests/ref_lib.py.  Test-side only: nothing in raingun_amd/ includes or loads it.
"""
import ctypes as C

import numpy as np

import ref_lib
from raingun_amd import _abi, aov
from raingun_amd.scene import SceneDesc
from ref_lib import c_camera, lib


def render(scene, width: int, height: int, cam=None, layers=aov.LAYERS, tile_rows: int = 0, stride: int = 1,
           offset: int = 0):
    """The reference's layers: (status, {layer: array}, counts dict, error_pixel)."""
    desc = scene if isinstance(scene, SceneDesc) else SceneDesc(scene)
    t = _abi.rg_tiling(tile_rows or height, stride, offset)
    rows = lib().rgo_tiling_rows(height, C.byref(t))
    out = {n: np.zeros(aov.layer_shape(n, rows, width), dtype=aov.DTYPES[n]) for n in layers}
    ptr = [out[n].ctypes.data if n in out else None for n in aov.LAYERS]
    counts = _abi.rg_ray_counts()
    err = C.c_int64(-1)
    cc = c_camera(cam) if cam is not None else None
    st = lib().rga_render(desc.ptr(), width, height, C.byref(t), C.byref(cc) if cc is not None else None, *ptr,
                          C.byref(counts), C.byref(err))
    return st, out, counts.as_dict(), int(err.value)


def cached(key, scene, width, height, cam=None, **tiling):
    """render() with every layer, computed once per key and handed out read-only."""
    k = ("aov", key, cam, width, height, tuple(sorted(tiling.items())))
    return ref_lib.cached(k, render, scene, width, height, cam, **tiling)


def bits(a: np.ndarray) -> np.ndarray:
    """The array's bit patterns (floats compare bit for bit: -0 is not +0, NaN equals itself)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def prime_rays(fov: float, width: int, height: int, fov_adjustment: float) -> np.ndarray:
    """create_prime's rays (ray.rs:37-54) of a frame in numpy f64, its expression order: (H*W, 6)."""
    x = np.arange(width, dtype=np.float64)[None, :]
    y = np.arange(height, dtype=np.float64)[:, None]
    aspect = np.float64(width) / np.float64(height)
    sx = np.broadcast_to(((((x + 0.5) / np.float64(width)) * 2.0 - 1.0) * aspect) * fov_adjustment, (height, width))
    sy = np.broadcast_to((1.0 - ((y + 0.5) / np.float64(height)) * 2.0) * fov_adjustment, (height, width))
    sz = np.full((height, width), -1.0)
    inv = 1.0 / np.sqrt((sx * sx + sy * sy) + sz * sz)
    rays = np.zeros((height, width, 6), dtype=np.float64)
    rays[..., 3], rays[..., 4], rays[..., 5] = sx * inv, sy * inv, sz * inv
    return rays.reshape(-1, 6)
