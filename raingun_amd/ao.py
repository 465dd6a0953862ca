"""Ambient occlusion: per pixel, the share of the hemisphere above the primary hit that is open, and the
picture both command lines write of it, restated in numpy.

The pass itself is DeviceScene.render_ao (rg_render_ao, csrc/rg_ao.hip; the arithmetic: csrc/rg_ao.h, the
contract: include/raingun.h): the primary ray rg_render_aov traces for the pixel, then samples x samples
any-hit rays from its hit, cosine-weighted about the normal facing the ray.  (H, W) float32: open / k^2,
1.0 on a miss.

* tables(k)      rg_ao_tables: the k*k points of the unit hemisphere, (k*k, 3) float64
* rotations()    rg_lens_tables' 64 turns, (64, 2) float64
* directions()   steps 3-7 of the contract in numpy f64, its expression order: the rays of the hit pixels
* visualize()    the numpy statement of `--ao`'s PNG (raingun_cli.cpp writes the same bytes): grey, the byte
                 is the Rust `(ao * 255.0) as u8` of color.py, alpha 255
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .aa import f32_to_u8

MAX_SAMPLES = 8
DEFAULT_BIAS = 1e-13  # the reference's own shadow bias

F32 = np.float32
F64 = np.float64


def tables(k: int) -> np.ndarray:
    """rg_ao_tables(k): the points (k*k, 3) as a float64 array (pure host code of the library)."""
    if not 1 <= int(k) <= MAX_SAMPLES:
        raise ValueError(f"samples must be 1..{MAX_SAMPLES} (got {k!r})")
    points = np.zeros((k * k, 3), F64)
    _abi.check(_abi.lib().rg_ao_tables(k, points.ctypes.data_as(C.POINTER(C.c_double))), "rg_ao_tables")
    return points


def rotations() -> np.ndarray:
    """rg_lens_tables' 64 turns (cos, sin) as a (64, 2) float64 array."""
    dp = C.POINTER(C.c_double)
    points = np.zeros(2, F64)
    rot = np.zeros((64, 2), F64)
    _abi.check(_abi.lib().rg_lens_tables(1, points.ctypes.data_as(dp), rot.ctypes.data_as(dp)), "rg_lens_tables")
    return rot


def parse_spec(spec: str):
    """`--ao`'s K[,RADIUS[,BIAS]] -> (samples, radius, bias); ValueError with the command lines' message."""
    parts = str(spec).split(",")
    try:
        if not 1 <= len(parts) <= 3 or any(p.strip() == "" for p in parts):
            raise ValueError
        k = int(parts[0])
        radius = float(parts[1]) if len(parts) > 1 else float("inf")
        bias = float(parts[2]) if len(parts) > 2 else DEFAULT_BIAS
    except ValueError:
        raise ValueError(f"--ao: expected K[,RADIUS[,BIAS]] (got {spec!r})") from None
    if not 1 <= k <= MAX_SAMPLES:
        raise ValueError(f"--ao: K must be 1..{MAX_SAMPLES} (got {k})")
    if not radius > 0.0:
        raise ValueError(f"--ao: RADIUS must be > 0 (got {parts[1]})")
    if not (np.isfinite(bias) and bias >= 0.0):
        raise ValueError(f"--ao: BIAS must be finite and >= 0 (got {parts[2]})")
    return k, radius, bias


def lowbias32(n) -> np.ndarray:
    """The hash of rg_lens (u32 wrap-around)."""
    n = np.asarray(n, dtype=np.uint64) & 0xFFFFFFFF
    n ^= n >> 16
    n = (n * 0x7FEB352D) & 0xFFFFFFFF
    n ^= n >> 15
    n = (n * 0x846CA68B) & 0xFFFFFFFF
    n ^= n >> 16
    return n.astype(np.uint32)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _normalize(v):
    return v * (1.0 / np.sqrt(_dot(v, v)))[..., None]


def directions(origin, direction, t, normal, pixel, samples: int, bias: float = DEFAULT_BIAS, points=None, turns=None):
    """The AO rays of N hit pixels (steps 2's h and 3-7 of include/raingun.h), f64 in the contract's order.

    origin, direction (N, 3): the primary rays; t (N,): their hit distances; normal (N, 3): surface_normal at
    the hit; pixel (N,): y * width + x.  Returns (O (N, 3), D (N, k*k, 3)): the rays' common origin and their
    normalised directions, sample j at D[:, j]."""
    o = np.asarray(origin, F64).reshape(-1, 3)
    d = np.asarray(direction, F64).reshape(-1, 3)
    t = np.asarray(t, F64).reshape(-1)
    n = np.asarray(normal, F64).reshape(-1, 3)
    pts = tables(samples) if points is None else np.asarray(points, F64)
    rot = rotations() if turns is None else np.asarray(turns, F64)
    with np.errstate(all="ignore"):
        h = o + d * t[:, None]
        m = _normalize(n)
        nf = np.where((_dot(m, d) <= 0.0)[:, None], m, -m)
        O = h + nf * F64(bias)
        s = np.copysign(1.0, nf[:, 2])
        a = -1.0 / (s + nf[:, 2])
        b = (nf[:, 0] * nf[:, 1]) * a
        T = np.stack([1.0 + (s * nf[:, 0]) * (nf[:, 0] * a), s * b, (-s) * nf[:, 0]], axis=1)
        B = np.stack([b, s + (nf[:, 1] * nf[:, 1]) * a, -nf[:, 1]], axis=1)
        turn = rot[lowbias32(pixel) & 63]
        c, g = turn[:, 0:1], turn[:, 1:2]
        Tr = c * T + g * B
        Br = c * B - g * T
        px, py, pz = (pts[None, :, k, None] for k in range(3))
        D = (Tr[:, None, :] * px + Br[:, None, :] * py) + nf[:, None, :] * pz
        D = _normalize(D)
    return O, D


def visualize(ao) -> np.ndarray:
    """The picture of an AO frame: (H, W, 4) uint8, grey u8(ao * 255.0f), alpha 255."""
    a = np.asarray(ao, dtype=F32)
    if a.ndim != 2:
        raise ValueError("ao: expected an array of shape (H, W)")
    out = np.zeros((*a.shape, 4), dtype=np.uint8)
    out[..., :3] = f32_to_u8(a * F32(255.0))[..., None]
    out[..., 3] = 255
    return out
