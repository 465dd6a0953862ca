"""The ambient term: the AO pass finished by an edge-stopping filter and multiplied into an ambient light,
restated in numpy in the contract's order (include/raingun.h at rg_ao_filter and rg_render_image_ambient; the
library's statement: csrc/rg_ambient.h; the kernels: csrc/rg_ao_filter.hip).

* filter_ao()    rg_ao_filter: the tent filter of an AO frame guided by the AOV pass's body and normal layers;
                 f32, unfused, taps dy outer / dx inner -- the GPU gives the same bits
* shares()       share[b] per body of a scene: diffuse albedo, reflecting (1 - reflectivity) * albedo, refractive 0
* compose()      the ambient term added to the clamped f32 means of the beauty frame, and the frame's bytes
* parse_spec()   `--ambient`'s R,G,B (or one number);  parse_filter_spec(): `--ao-filter`'s R[,NMIN]

DeviceScene.filter_ao and DeviceScene.render_ambient run the library's versions.
"""
from __future__ import annotations

import numpy as np

from .aa import f32_to_u8

import re

F32 = np.float32
_DECIMAL = re.compile(r"[0-9.eE+-]+\Z")  # a number of the two flags: what both command lines accept, no more
_F32_MAX = float(np.finfo(np.float32).max)


def _number(text: str) -> float:
    """A decimal number within f32's range (no inf, nan, hex floats or digit underscores); ValueError otherwise."""
    if not _DECIMAL.match(text):
        raise ValueError(text)
    v = float(text)
    if not abs(v) <= _F32_MAX:
        raise ValueError(text)
    return v

MAX_RADIUS = 8
DEFAULT_FILTER = (2, 0.9)  # `--ao-filter`'s default when `--ambient` is given


def filter_ao(ao, body, normal, radius: int, normal_min: float, reverse: bool = False) -> np.ndarray:
    """rg_ao_filter in numpy: (H, W) f32, (H, W) i32, (H, W, 3) f32 -> (H, W) f32.

    reverse=True walks the taps in the opposite order (not the contract: tests use it to show that the order
    matters)."""
    a = np.ascontiguousarray(ao, dtype=F32)
    b = np.ascontiguousarray(body, dtype=np.int32)
    n = np.ascontiguousarray(normal, dtype=F32)
    if a.ndim != 2 or a.size == 0 or b.shape != a.shape or n.shape != (*a.shape, 3):
        raise ValueError("expected ao (H, W), body (H, W) and normal (H, W, 3)")
    r = int(radius)
    nmin = F32(normal_min)
    if not 1 <= r <= MAX_RADIUS:
        raise ValueError(f"radius must be 1..{MAX_RADIUS} (got {radius!r})")
    if not (nmin >= 0 and nmin <= 1):
        raise ValueError(f"normal_min must be in [0, 1] (got {normal_min!r})")
    H, W = a.shape
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    taps = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]
    if reverse:
        taps.reverse()
    with np.errstate(all="ignore"):
        nn = (nx * nx + ny * ny) + nz * nz
        t = np.full((), nmin * nmin, dtype=F32)
        acc_sum = np.zeros((H, W), F32)
        wsum = np.zeros((H, W), np.int32)
        for dy, dx in taps:
            y0, y1 = max(0, -dy), min(H, H - dy)
            x0, x1 = max(0, -dx), min(W, W - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            c = (slice(y0, y1), slice(x0, x1))                       # the centres whose tap lies in the frame
            q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))   # their taps
            w = (r + 1 - abs(dx)) * (r + 1 - abs(dy))
            if dy == 0 and dx == 0:
                ok = np.ones((y1 - y0, x1 - x0), bool)
            else:
                d = (nx[c] * nx[q] + ny[c] * ny[q]) + nz[c] * nz[q]
                ok = (b[q] == b[c]) & (d > F32(0.0)) & (d * d >= t * (nn[c] * nn[q]))
            acc_sum[c] = np.where(ok, acc_sum[c] + F32(w) * a[q], acc_sum[c])
            wsum[c] += np.where(ok, np.int32(w), np.int32(0))
        out = np.where(b < 0, a, acc_sum / wsum.astype(F32))
    return out.astype(F32, copy=False)


def share(surface: str, albedo: float, reflectivity: float = 0.0) -> np.float32:
    """share of one material (f32, unfused)."""
    if surface == "Diffuse":
        return F32(albedo)
    if surface == "Reflecting":
        return (F32(1.0) - F32(reflectivity)) * F32(albedo)
    if surface == "Refractive":
        return F32(0.0)
    raise ValueError(f"unknown surface {surface!r}")


def shares(scene) -> np.ndarray:
    """share[b] for every body of a raingun_amd.scene.Scene, in YAML order: (n_bodies,) float32."""
    return np.array([share(b.material.surface, b.material.albedo, b.material.reflectivity) for b in scene.bodies],
                    dtype=F32).reshape(-1)


def _clamp(v: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return np.where((v >= 0) & (v <= 1), v, np.where(v > 1, F32(1.0), F32(0.0))).astype(F32)


def compose(rgb, albedo, body, aof, share_table, color):
    """The compose of rg_render_image_ambient: rgb (H, W, 3) the clamped f32 means of the beauty frame, albedo
    (H, W, 3) and body (H, W) the AOV layers, aof (H, W) the filtered (or raw) AO pass, share_table (n_bodies,),
    color three floats.  Returns ((H, W, 3) float32 clamped colours, (H, W, 4) uint8 frame)."""
    rgb = np.asarray(rgb, dtype=F32)
    albedo = np.asarray(albedo, dtype=F32)
    body = np.asarray(body, dtype=np.int32)
    aof = np.asarray(aof, dtype=F32)
    table = np.asarray(share_table, dtype=F32).reshape(-1)
    col = np.broadcast_to(np.asarray(color, dtype=F32).reshape(-1), (3,))
    hit = body >= 0
    with np.errstate(all="ignore"):
        k = np.where(hit, table[np.where(hit, body, 0)] if table.size else F32(0.0), F32(0.0)).astype(F32) * aof
        v = np.where(hit[..., None], rgb + (col[None, None, :] * albedo) * k[..., None], rgb).astype(F32)
        v = _clamp(v)
        rgba = np.empty((*body.shape, 4), dtype=np.uint8)
        rgba[..., :3] = f32_to_u8(v * F32(255.0))
    rgba[..., 3] = 255
    return v, rgba


def parse_spec(spec: str):
    """`--ambient`'s R,G,B (or one number for grey) -> (r, g, b) floats; ValueError with the command lines' message."""
    parts = str(spec).split(",")
    try:
        if len(parts) not in (1, 3) or any(p == "" or p != p.strip() for p in parts):
            raise ValueError
        vals = [_number(p) for p in parts]
    except ValueError:
        raise ValueError(f"--ambient: expected R,G,B or one number (got {spec!r})") from None
    if len(vals) == 1:
        vals = vals * 3
    f = [F32(v) for v in vals]
    if not all(np.isfinite(v) and v >= 0 for v in f):
        raise ValueError(f"--ambient: the colour must be finite and >= 0 (got {spec!r})")
    return tuple(float(v) for v in f)


def parse_filter_spec(spec: str):
    """`--ao-filter`'s R[,NMIN] -> (radius, normal_min); radius 0: no filter.  ValueError with the command lines'
    message."""
    parts = str(spec).split(",")
    try:
        if not 1 <= len(parts) <= 2 or any(p == "" or p != p.strip() for p in parts):
            raise ValueError
        if not parts[0].lstrip("+").isdigit() or not parts[0].isascii() or parts[0].count("+") > 1:
            raise ValueError
        r = int(parts[0])
        nmin = _number(parts[1]) if len(parts) > 1 else DEFAULT_FILTER[1]
    except ValueError:
        raise ValueError(f"--ao-filter: expected R[,NMIN] (got {spec!r})") from None
    if not 0 <= r <= MAX_RADIUS:
        raise ValueError(f"--ao-filter: R must be 0..{MAX_RADIUS} (got {r})")
    if not (F32(nmin) >= 0 and F32(nmin) <= 1):
        raise ValueError(f"--ao-filter: NMIN must be in [0, 1] (got {parts[1]})")
    return r, float(F32(nmin))
