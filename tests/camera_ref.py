"""The reference for camera frames, shared by tests/test_camera_cpu.py and tests/test_gpu_camera.py.

tests/native/camera_oracle.c (the pinned oracle plus rgo_render's pixel loop with the camera ray) is
built into a temporary directory with the oracle's own flags, read from oracle/Makefile, and loaded
with ctypes.  Test-side only: nothing in raingun_amd/ includes or loads it.  Also here: the scene
mirrored in x and z (the 180-degree fact), and the scenes and poses the two modules share.
"""
import copy
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np

from raingun_amd import _abi
from raingun_amd.camera import Camera
from raingun_amd.scene import AABB, DirectionalLight, Disk, Plane, SceneDesc, Sphere, SphericalLight

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "native" / "camera_oracle.c"
REQUIRED_FLAGS = ("-O2", "-std=c11", "-ffp-contract=off", "-fno-fast-math")

IDENTITY = Camera.identity()
TURNED = Camera(eye=(0.0, 0.0, 0.0), right=(-1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), forward=(0.0, 0.0, 1.0))  # 180 deg about y

_LIB = None
_TMP = None


def oracle_flags():
    """CC and CFLAGS of oracle/Makefile (the `?=` defaults)."""
    text = (REPO / "oracle" / "Makefile").read_text()
    cc = re.search(r"^CC\s*\?=\s*(.+)$", text, re.M).group(1).strip()
    flags = re.search(r"^CFLAGS\s*\?=\s*(.+)$", text, re.M).group(1).split()
    for f in REQUIRED_FLAGS:
        assert f in flags, (f, flags)
    return cc, flags


def lib():
    global _LIB, _TMP
    if _LIB is None:
        _TMP = tempfile.TemporaryDirectory(prefix="camera_oracle_")
        out = Path(_TMP.name) / "libcamera_oracle.so"
        cc, flags = oracle_flags()
        subprocess.run([cc, *flags, "-shared", "-pthread", "-o", str(out), str(SRC), "-lm"], check=True, timeout=300)
        l = C.CDLL(str(out))
        P = C.POINTER
        l.rgc_render.restype = C.c_int32
        l.rgc_render.argtypes = [P(_abi.rg_scene_desc), C.c_uint32, C.c_uint32, P(_abi.rg_tiling), P(_abi.rg_camera),
                                 C.c_void_p, C.c_void_p, P(_abi.rg_ray_counts), P(C.c_int64)]
        l.rgo_tiling_rows.restype = C.c_uint32
        l.rgo_tiling_rows.argtypes = [C.c_uint32, P(_abi.rg_tiling)]
        _LIB = l
    return _LIB


def c_camera(cam: Camera) -> _abi.rg_camera:
    return _abi.rg_camera((C.c_double * 3)(*cam.eye), (C.c_double * 3)(*cam.right), (C.c_double * 3)(*cam.up),
                          (C.c_double * 3)(*cam.forward))


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


_CACHE = {}


def cached(key, scene, cam, width, height, **tiling):
    """render(), computed once per key and handed out read-only."""
    k = (key, cam, width, height, tuple(sorted(tiling.items())))
    if k not in _CACHE:
        st, rgba, rgb, counts, err = render(scene, cam, width, height, **tiling)
        rgba.setflags(write=False)
        rgb.setflags(write=False)
        _CACHE[k] = (st, rgba, rgb, counts, err)
    return _CACHE[k]


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
