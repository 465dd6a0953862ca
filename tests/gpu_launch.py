"""What the GPU test modules share: the device check, the CPU restatement's frames, the device-resident
launch with its debug queries, the pixel comparison, and a few constants and helpers.  A plain module:
fixtures stay in the test modules and call into it.
"""
import ctypes as C
import subprocess
from collections import namedtuple

import numpy as np

from raingun_amd import _abi, _host
from raingun_amd.color import Color
from raingun_amd.scene import DirectionalLight, Material, Scene, SceneDesc, Sphere

SIZES = [(97, 61), (64, 40)]  # partial 8x8 tiles at the right and bottom edges; whole tiles


def require_device():
    """The body of every module's autouse `_device` fixture."""
    lib = _abi.lib()  # raises if the HIP library is missing: no fallback
    assert lib.rg_device_count() > 0, "no HIP device visible"


def any_scene():
    """One sphere under one light, for the debug entries that need a scene handle and nothing of the scene."""
    return Scene(bodies=[Sphere((0.0, 0.0, -5.0), 1.0, Material(Color.from_str("#ffffff"), 0.5))],
                 lights=[DirectionalLight((0.0, -1.0, -1.0), Color.from_str("#ffffff"), 1.0)])


_ORACLE = {}


def oracle_frame(oracle_lib, key, scene, w, h):
    """The CPU restatement's whole frame and ray counts -> (rgba, counts), computed once per (key, size) and
    handed out read-only.  One cache for all modules: a key names one scene everywhere."""
    k = (key, w, h)
    if k not in _ORACLE:
        o_st, o_rgba, _, o_counts, _ = oracle_lib.render(SceneDesc(scene), w, h)
        assert o_st == 0, f"the CPU restatement reports status {o_st}"
        o_rgba.setflags(write=False)
        _ORACLE[k] = (o_rgba, o_counts)
    return _ORACLE[k]


Launch = namedtuple("Launch", "rgba counts plain shadow_volume")


def device_launch(ds, w, h, mode="single", tiling=None, want_rgb=False, stream=None):
    """One device-resident launch (the whole frame, or the rows of `tiling`) into a buffer pre-filled with 7
    -> Launch(rgba rows, ray counts, ran PLAIN, ran with the shadow volume).  "single" is
    rg_render_tiles_async with stats, "pipelined" rg_render_tiles_pipelined and the debug counters."""
    import torch

    lib = _abi.lib()
    t = tiling if tiling is not None else _abi.rg_tiling(h, 1, 0)
    rows = lib.rg_tiling_rows(h, C.byref(t))
    rgba = torch.full((rows, w, 4), 7, dtype=torch.uint8, device="cuda")
    rgb = torch.zeros((rows, w, 3), dtype=torch.float32, device="cuda") if want_rgb else None
    sp = C.c_void_p(stream.cuda_stream) if stream is not None else None
    rp = C.c_void_p(rgb.data_ptr()) if want_rgb else None
    if mode == "single":
        st = _abi.rg_stats()
        _abi.check(lib.rg_render_tiles_async(ds.handle, w, h, C.byref(t), C.c_void_p(rgba.data_ptr()), rp, sp,
                                             C.byref(st)))
        counts = st.rays.as_dict()
    else:
        assert mode == "pipelined", mode
        _abi.check(lib.rg_render_tiles_pipelined(ds.handle, w, h, C.byref(t), C.c_void_p(rgba.data_ptr()), rp, sp))
        torch.cuda.synchronize()
        words = (C.c_uint64 * 16)()
        _abi.check(lib.rg_debug_counters(ds.handle, words))
        assert words[3] == 0, "the launch reported an error"
        counts = {"primary": words[0], "shadow": words[1], "secondary": words[2]}
    plain, used = ds.last_plain(), ds.last_shadow_volume()
    torch.cuda.synchronize()
    return Launch(rgba.cpu().numpy(), counts, plain, used)


def assert_same_pixels(got, want, what=""):
    mism = int(np.count_nonzero((got != want).any(axis=2)))
    assert mism == 0, f"{what + ': ' if what else ''}{mism} RGBA8 pixels differ"


def png(path):
    from PIL import Image

    return np.asarray(Image.open(path).convert("RGBA"))


def native_cli_path():
    """The `raingun` binary, built if it is missing."""
    if not _host.CLI_PATH.exists():
        subprocess.run(["make", "-s", "-C", str(_host.SRC_DIR)], check=True)
    return str(_host.CLI_PATH)
