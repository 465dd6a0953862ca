"""The reference library of the tests: tests/native/ref_frames.c (the pinned oracle plus one pixel loop under
the camera, AOV and lens entries), built once per session into a temporary directory with the oracle's own
flags, read from oracle/Makefile, and loaded with ctypes.  Test-side only: nothing in raingun_amd/ includes
or loads it.  tests/camera_ref.py, aov_ref.py and lens_ref.py call its entries.
"""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np

from raingun_amd import _abi
from raingun_amd.camera import Camera

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "native" / "ref_frames.c"
REQUIRED_FLAGS = ("-O2", "-std=c11", "-ffp-contract=off", "-fno-fast-math")

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
        _TMP = tempfile.TemporaryDirectory(prefix="ref_frames_")
        out = Path(_TMP.name) / "libref_frames.so"
        cc, flags = oracle_flags()
        subprocess.run([cc, *flags, "-shared", "-pthread", "-o", str(out), str(SRC), "-lm"], check=True, timeout=300)
        l = C.CDLL(str(out))
        P = C.POINTER
        frame = [P(_abi.rg_scene_desc), C.c_uint32, C.c_uint32]
        tail = [P(_abi.rg_ray_counts), P(C.c_int64)]
        l.rgc_render.restype = l.rga_render.restype = l.rgl_render.restype = C.c_int32
        l.rgc_render.argtypes = [*frame, P(_abi.rg_tiling), P(_abi.rg_camera), C.c_void_p, C.c_void_p, *tail]
        l.rga_render.argtypes = [*frame, P(_abi.rg_tiling), P(_abi.rg_camera), *[C.c_void_p] * 5, *tail]
        l.rgl_render.argtypes = [*frame, C.c_uint32, P(_abi.rg_camera), C.c_double, C.c_double, P(C.c_double),
                                 P(C.c_double), C.c_void_p, C.c_void_p, *tail]
        l.rgo_tiling_rows.restype = C.c_uint32
        l.rgo_tiling_rows.argtypes = [C.c_uint32, P(_abi.rg_tiling)]
        _LIB = l
    return _LIB


def c_camera(cam: Camera) -> _abi.rg_camera:
    return _abi.rg_camera((C.c_double * 3)(*cam.eye), (C.c_double * 3)(*cam.right), (C.c_double * 3)(*cam.up),
                          (C.c_double * 3)(*cam.forward))


_CACHE = {}


def cached(key, fn, *args, **kwargs):
    """fn(*args, **kwargs), computed once per key; its arrays (in the tuple, or in a dict in it) read-only."""
    if key not in _CACHE:
        result = fn(*args, **kwargs)
        for item in result:
            for a in (item.values() if isinstance(item, dict) else (item,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _CACHE[key] = result
    return _CACHE[key]
