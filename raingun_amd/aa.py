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

The render itself is DeviceScene.render_image_aa (rg_render_image_aa).  The adaptive form
(DeviceScene.render_image_aa_adaptive, rg_render_image_aa_adaptive) is restated at the end:
edge_mask and resolve_adaptive.
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


# ---------------------------------------------------------------- adaptive
# Adaptive anti-aliasing (rg_render_image_aa_adaptive): the k x k samples are traced only for
# the pixels on edges of the 1-sample frame.  The arithmetic of rg_edge_mask_kernel
# (csrc/rg_edge.hip) and rg_resolve_adaptive_kernel (csrc/rg_resolve.hip):
#
# * contrast  m(p) = max |base[p][c] - base[q][c]| as integers, over c in {R, G, B} and over the
#             up to eight neighbours q of p inside the frame; 0 without neighbours; alpha ignored
# * mask      flag(p) = m(p) >= threshold (0..256): symmetric, so both sides of an edge are flagged
# * pixel     flagged: the box resolve of its k x k samples (resolve_box); unflagged: the base
#             pixel's bytes and clamp_sample(base f32 RGB), the k = 1 resolve
MAX_THRESHOLD = 256


def edge_mask(rgba: np.ndarray, threshold: int) -> np.ndarray:
    """(H, W, 4) uint8 RGBA -> (H, W) uint8 mask, 1 where the 8-neighbourhood contrast >= threshold."""
    t = int(threshold)
    if not 0 <= t <= MAX_THRESHOLD:
        raise ValueError(f"threshold must be between 0 and {MAX_THRESHOLD}")
    rgba = np.asarray(rgba, dtype=np.uint8)
    if rgba.ndim != 3 or rgba.shape[2] != 4 or rgba.size == 0:
        raise ValueError("expected (height, width, 4) uint8 RGBA")
    h, w = rgba.shape[:2]
    c = rgba[..., :3].astype(np.int32)
    m = np.zeros((h, w), dtype=np.int32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if (dy == 0 and dx == 0) or abs(dy) >= h or abs(dx) >= w:
                continue
            # p in [y0, y1) x [x0, x1) has its neighbour q = p + (dy, dx) inside the frame
            y0, y1 = max(0, -dy), min(h, h - dy)
            x0, x1 = max(0, -dx), min(w, w - dx)
            d = np.abs(c[y0:y1, x0:x1] - c[y0 + dy:y1 + dy, x0 + dx:x1 + dx]).max(axis=2)
            m[y0:y1, x0:x1] = np.maximum(m[y0:y1, x0:x1], d)
    return (m >= t).astype(np.uint8)


def resolve_adaptive(base_rgba: np.ndarray, base_rgb: np.ndarray, samples_rgb: np.ndarray, k: int,
                     threshold: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The adaptive frame from the 1-sample frame ((H, W, 4) uint8 and (H, W, 3) float32) and the
    (k H, k W, 3) float32 sample frame: ((H, W, 3) float32, (H, W, 4) uint8, (H, W) uint8 mask)."""
    base_rgba = np.asarray(base_rgba, dtype=np.uint8)
    base_rgb = np.asarray(base_rgb, dtype=np.float32)
    mask = edge_mask(base_rgba, threshold)
    if base_rgb.shape != base_rgba.shape[:2] + (3,):
        raise ValueError("expected (height, width, 3) float32 beside the RGBA frame")
    s_mean, s_rgba = resolve_box(samples_rgb, k)
    if s_rgba.shape != base_rgba.shape:
        raise ValueError("expected (samples*height, samples*width, 3) float32 samples")
    flagged = mask.astype(bool)
    mean = np.where(flagged[..., None], s_mean, clamp_sample(base_rgb)).astype(np.float32)
    rgba = np.where(flagged[..., None], s_rgba, base_rgba).astype(np.uint8)
    return mean, rgba, mask
