"""The reference for camera frames, shared by tests/test_camera_cpu.py and tests/test_gpu_camera.py.

rgc_render of tests/native/ref_frames.c (the pinned oracle plus rgo_render's pixel loop with the camera ray),
through tests/ref_lib.py.  Test-side only: nothing in raingun_amd/ includes or loads it.  Also here: the scene
mirrored in x and z (the 180-degree fact), and the poses the two modules share.
"""
import copy
import ctypes as C

import numpy as np

import ref_lib
from raingun_amd import _abi
from raingun_amd.camera import Camera
from raingun_amd.scene import AABB, DirectionalLight, Disk, Plane, SceneDesc, Sphere, SphericalLight
from ref_lib import c_camera, lib

IDENTITY = Camera.identity()
TURNED = Camera(eye=(0.0, 0.0, 0.0), right=(-1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), forward=(0.0, 0.0, 1.0))  # 180 deg about y


def render(scene, cam: Camera, width: int, height: int, tile_rows: int = 0, stride: int = 1, offset: int = 0):
    """The camera reference's frame: (status, rgba, rgb, counts dict, error_pixel), as oracle.render."""
    desc = scene if isinstance(scene, SceneDesc) else SceneDesc(scene)
    t = _abi.rg_tiling(tile_rows or height, stride, offset)
    rows = lib().rgo_tiling_rows(height, C.byref(t))
    rgba = np.zeros((rows, width, 4), dtype=np.uint8)
    rgb = np.zeros((rows, width, 3), dtype=np.float32)
    counts = _abi.rg_ray_counts()
    err = C.c_int64(-1)
    cc = c_camera(cam)
    st = lib().rgc_render(desc.ptr(), width, height, C.byref(t), C.byref(cc), rgba.ctypes.data, rgb.ctypes.data,
                          C.byref(counts), C.byref(err))
    return st, rgba, rgb, counts.as_dict(), int(err.value)


def cached(key, scene, cam, width, height, **tiling):
    """render(), computed once per key and handed out read-only."""
    k = ("camera", key, cam, width, height, tuple(sorted(tiling.items())))
    return ref_lib.cached(k, render, scene, cam, width, height, **tiling)


def _flip(v):
    return (-v[0], v[1], -v[2])


def mirrored_xz(scene):
    """The scene with every x and z coordinate negated: body positions, normals, light vectors and AABB
    corners (re-sorted into min and max).  Negation is exact."""
    s = copy.copy(scene)
    s.bodies, s.lights = [], []
    for b in scene.bodies:
        b = copy.copy(b)
        if isinstance(b, Sphere):
            b.center = _flip(b.center)
        elif isinstance(b, (Plane, Disk)):
            b.origin, b.normal = _flip(b.origin), _flip(b.normal)
        elif isinstance(b, AABB):
            lo, hi = _flip(b.bounds[0]), _flip(b.bounds[1])
            b.bounds = (tuple(min(p, q) for p, q in zip(lo, hi)), tuple(max(p, q) for p, q in zip(lo, hi)))
        else:
            raise TypeError(b)
        s.bodies.append(b)
    for l in scene.lights:
        l = copy.copy(l)
        if isinstance(l, DirectionalLight):
            l.direction = _flip(l.direction)
        elif isinstance(l, SphericalLight):
            l.position = _flip(l.position)
        else:
            raise TypeError(l)
        s.lights.append(l)
    return s
