"""AOV layers (auxiliary output variables, a G-buffer): what lies under each pixel, and the pictures
both command lines write of them, restated in numpy.

The layers themselves are DeviceScene.render_aov (rg_render_aov, csrc/rg_aov.hip): one primary ray per
pixel, the ray rg_render_image traces for that pixel.

* body    (H, W)    int32    YAML index of the primary hit, -1 on a miss
* depth   (H, W)    float64  its Scene::trace distance, +inf on a miss
* normal  (H, W, 3) float32  the reference's geometric normal at the hit, 0,0,0 on a miss
* uv      (H, W, 2) float32  texture_coords at the hit before the material's offsets, 0,0 on a miss
* albedo  (H, W, 3) float32  Material::color at the hit, the scene's default colour on a miss

visualize() is the numpy statement of `--aov`'s PNGs (raingun_cli.cpp writes the same bytes), as
aa.py is for the resolve: every cast is the Rust `f32 as u8` of color.py, alpha is 255.
"""
from __future__ import annotations

import numpy as np

from .aa import f32_to_u8

LAYERS = ("body", "depth", "normal", "uv", "albedo")
DTYPES = {"body": np.int32, "depth": np.float64, "normal": np.float32, "uv": np.float32, "albedo": np.float32}
CHANNELS = {"body": 0, "depth": 0, "normal": 3, "uv": 2, "albedo": 3}  # 0: a scalar per pixel
BODY_HASH = 2654435761  # Knuth's multiplicative hash, mod 2^32

F32 = np.float32


def parse_layers(spec) -> tuple:
    """A comma list (or a sequence) of layer names, or "all" -> the names in LAYERS order, each once."""
    names = list(LAYERS) if spec == "all" else spec.split(",") if isinstance(spec, str) else list(spec)
    if not names or any(n not in LAYERS for n in names):
        raise ValueError(f"--aov: expected a comma list of {', '.join(LAYERS)}, or all (got {spec!r})")
    return tuple(n for n in LAYERS if n in names)


def layer_shape(layer: str, rows: int, width: int) -> tuple:
    return (rows, width, CHANNELS[layer]) if CHANNELS[layer] else (rows, width)


def _rgba(h: int, w: int) -> np.ndarray:
    out = np.zeros((h, w, 4), dtype=np.uint8)
    out[..., 3] = 255
    return out


def visualize(layer: str, array) -> np.ndarray:
    """The picture of one layer: (H, W, 4) uint8, alpha 255.

    body    h = uint32(id + 1) * 2654435761; bytes h >> 24, (h >> 16) & 255, (h >> 8) & 255; a miss is black
    depth   over the frame's finite hits, in f64, v = 1 - (t - tmin) / (tmax - tmin) (1 when tmax == tmin);
            grey u8((f32)v * 255.0f); a miss is black
    normal  u8((n_k * 0.5f + 0.5f) * 255.0f); a miss (0,0,0) is black
    uv      R, G = u8((c - floorf(c)) * 255.0f), B = 0
    albedo  u8(c * 255.0f) (color.rs:32-37)
    """
    if layer not in LAYERS:
        raise ValueError(f"unknown AOV layer {layer!r}")
    a = np.asarray(array, dtype=DTYPES[layer])
    want = 3 if CHANNELS[layer] else 2
    if a.ndim != want or (CHANNELS[layer] and a.shape[2] != CHANNELS[layer]):
        raise ValueError(f"{layer}: expected an array of shape {layer_shape(layer, 'H', 'W')}")
    out = _rgba(a.shape[0], a.shape[1])
    if layer == "body":
        hit = a >= 0
        h = ((a.astype(np.int64) + 1) * BODY_HASH) & 0xFFFFFFFF
        for k, shift in enumerate((24, 16, 8)):
            out[..., k] = np.where(hit, (h >> shift) & 255, 0).astype(np.uint8)
    elif layer == "depth":
        hit = np.isfinite(a)
        if hit.any():
            tmin, tmax = a[hit].min(), a[hit].max()
            with np.errstate(invalid="ignore", over="ignore"):
                v = np.where(hit, 1.0 - (a - tmin) / (tmax - tmin), 0.0) if tmax != tmin else np.where(hit, 1.0, 0.0)
            grey = f32_to_u8(v.astype(F32) * F32(255.0))
            out[..., :3] = np.where(hit, grey, 0).astype(np.uint8)[..., None]
    elif layer == "normal":
        hit = (a != 0).any(axis=2)
        byte = f32_to_u8((a * F32(0.5) + F32(0.5)) * F32(255.0))
        out[..., :3] = np.where(hit[..., None], byte, 0)
    elif layer == "uv":
        with np.errstate(invalid="ignore"):
            out[..., :2] = f32_to_u8((a - np.floor(a)) * F32(255.0))
    else:
        out[..., :3] = f32_to_u8(a * F32(255.0))
    return out
