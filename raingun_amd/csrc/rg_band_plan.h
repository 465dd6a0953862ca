// rg_band_plan.h — how a frame is cut into row bands (host-visible frames, rg_capi.hip;
// supersampled frames, rg_aa.hip) and the constants that decide it.  Plain integer
// arithmetic, no HIP: tests/native/band_plan_test.cpp checks it on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#define RG_IMAGE_MAX_BANDS 16        // row bands of a host-visible frame at most (rg_debug_set_image_bands)
#define RG_IMAGE_BAND_PX (2u << 20)  // ~pixels per band of a banded host-visible frame
#ifndef RG_AA_SLOT_BYTES
// supersampled frames (rg_aa.hip): the scratch of one band of samples (RGBA8 + f32 RGB,
// 16 B per sample) stays within this; two such slots, one per render stream
#define RG_AA_SLOT_BYTES ((size_t)64 << 20)
#endif
#ifndef RG_AA_ADAPTIVE_SLOT_BYTES
// adaptive anti-aliasing (rg_aa.hip "adaptive"): its bands' sparse launches hold a fraction of a
// band's tiles, so they want larger bands: 4K, k = 4, T = 32 at 64 / 136 / 272 / 544 output rows
// per band: test1 4.26 / 3.29 / 2.88 / 2.64 ms, north star 16.7 / 12.6 / 10.7 / 10.0 ms
// (DESIGN.md 4p); 256 MiB is 272 rows there
#define RG_AA_ADAPTIVE_SLOT_BYTES ((size_t)256 << 20)
#endif
#define RG_AA_MIN_BAND_ROWS 8  // output rows per band at least (automatic choice)

// `bands` bands of `band_rows` rows of `width` pixels cover host rows [0, host_rows): band b
// holds rows [b band_rows, min(host_rows, (b + 1) band_rows)).
struct rg_band_plan {
    uint32_t width, band_rows, bands, host_rows;
};

inline uint32_t rg_band_rows(const rg_band_plan &p, uint32_t b) {
    const uint32_t r0 = b * p.band_rows;
    return std::min(p.host_rows, r0 + p.band_rows) - r0;
}

// A frame delivered whole (a sharded tiling's one launch).
inline rg_band_plan rg_one_band(uint32_t W, uint32_t rows) { return {W, rows, 1u, rows}; }

// Bands of a banded host-visible frame: the first band's copy starts while
// the later bands render (the frame's PCIe transfer alone: ~0.59 ms for 33 MB
// at the measured 56 GB/s, profiles/r02/host_visible/d2h_probe.jsonl).  ~band_px pixels
// per band, at most 3: a 4K frame in 3 bands 0.95 ms, in 16 bands 1.46 ms --
// small launches leave most of the GPU idle (hv_sweep_bands_before.jsonl).
// forced > 0 (rg_debug_set_image_bands) overrides.  Whole 8x8 tiles per band, so fewer
// bands than asked may cover the frame.
inline rg_band_plan rg_image_band_plan(int forced, uint32_t W, uint32_t H, size_t band_px) {
    uint32_t K = forced > 0 ? (uint32_t)forced
                            : (uint32_t)std::max<size_t>(1, std::min<size_t>(3, (size_t)H * W / band_px));
    uint32_t BR = (H + K - 1) / K;
    BR = (BR + 7u) & ~7u;
    K = (H + BR - 1) / BR;
    return {W, BR, K, H};
}

// Bands of a supersampled frame of k x k samples per pixel: one band's samples (k band_rows
// rows of k W samples, 16 B each) within slot_bytes, whole 8-row tile rows, at least min_rows;
// forced_rows > 0 (rg_debug_set_aa_band_rows) overrides.
inline rg_band_plan rg_aa_band_plan(int forced_rows, uint32_t W, uint32_t H, uint32_t k, size_t slot_bytes,
                                    uint32_t min_rows) {
    uint32_t rb;
    if (forced_rows > 0) {
        rb = (uint32_t)forced_rows;
    } else {
        const size_t per_row = (size_t)k * k * W * 16;
        rb = (uint32_t)std::min<size_t>(slot_bytes / per_row, 0x10000u) & ~7u;
        rb = std::max(rb, min_rows);
    }
    rb = std::min(rb, H);
    return {W, rb, (H + rb - 1) / rb, H};
}
