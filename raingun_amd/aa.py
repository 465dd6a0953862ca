"""Supersampled anti-aliasing: the box resolve of samples x samples f32 RGB
samples per pixel, restated in numpy.

This is the arithmetic of rg_resolve_kernel (csrc/rg_resolve.hip), operation for
operation, and the reference the tests hold the kernel to bit for bit.  Per
output pixel (x, y), channel c and k = samples:

* samples   s[j][i] = rgb[k y + j][k x + i][c]
* clamp     s' = s if 0 <= s <= 1; 1 if s > 1; 0 otherwise (negatives and NaN),
            which makes k = 1 the saturating `as u8` of Color::rgba (color.rs:32-37)
* sum       acc = 0, then acc = acc + s'[j][i] in float32, j outer, i inner
* mean      acc / float32(k k)
* byte      `(mean * 255.0) as u8`, alpha 255

The render itself is DeviceScene.render_image_aa (rg_render_image_aa).
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

MAX_SAMPLES = 8


def f32_to_u8(v: np.ndarray) -> np.ndarray:
    """Rust `f32 as u8`: truncate, saturate, NaN -> 0."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        inside = np.where(v > 0, np.minimum(v, np.float32(255.0)), np.float32(0.0))
    return inside.astype(np.uint8)


def clamp_sample(s: np.ndarray) -> np.ndarray:
    s = np.asarray(s, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where((s >= 0) & (s <= 1), s, np.where(s > 1, np.float32(1.0), np.float32(0.0))).astype(np.float32)


def resolve_box(rgb: np.ndarray, samples: int) -> Tuple[np.ndarray, np.ndarray]:
    """(k H, k W, 3) float32 samples -> ((H, W, 3) float32 means, (H, W, 4) uint8 RGBA)."""
    k = int(samples)
    if not 1 <= k <= MAX_SAMPLES:
        raise ValueError(f"samples must be between 1 and {MAX_SAMPLES}")
    rgb = np.asarray(rgb, dtype=np.float32)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.shape[0] % k or rgb.shape[1] % k or rgb.size == 0:
        raise ValueError("expected (samples*height, samples*width, 3) float32 samples")
    h, w = rgb.shape[0] // k, rgb.shape[1] // k
    s = clamp_sample(rgb)
    acc = np.zeros((h, w, 3), dtype=np.float32)
    for j in range(k):          # one float32 addition per sample plane, in the kernel's order:
        for i in range(k):      # np.sum / np.mean would add pairwise
            acc = acc + s[j::k, i::k, :]
    mean = (acc / np.float32(k * k)).astype(np.float32)
    rgba = np.empty((h, w, 4), dtype=np.uint8)
    rgba[..., :3] = f32_to_u8(mean * np.float32(255.0))
    rgba[..., 3] = 255
    return mean, rgba
