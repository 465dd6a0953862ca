// rg_sample_tiles.h — the 8x8 sample tiles of one band of a supersampled frame and the
// output pixels each of them overlaps (adaptive anti-aliasing: rg_edge.hip lists the tiles
// that hold a sample of a flagged pixel, rg_aa.hip launches the list).  A band of `rows`
// output rows of `W` pixels with k x k samples each is rendered as a launch of its own, k W
// samples wide and k rows sample rows high; its tiles are local to that launch: tile t covers
// sample columns [8 tx, 8 tx + 8) and sample rows [8 ty, 8 ty + 8) of the band, clipped to it,
// with tx = t % tiles_x and ty = t / tiles_x.  Plain integer arithmetic usable from host and
// device: tests/native/sample_tiles_test.cpp checks it on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define RG_ST_HD __host__ __device__ inline
#else
#define RG_ST_HD inline
#endif

#define RG_SAMPLE_TILE 8u  // the render kernel's 8x8 tiles (RgKernelArgs::tile_wlog 3)

// Output pixels [x0, x1) x [y0, y1), rows counted from the band's first row.
struct rg_px_rect {
    uint32_t x0, x1, y0, y1;
};

RG_ST_HD uint32_t rg_sample_tiles_x(uint32_t W, uint32_t k) { return (k * W + RG_SAMPLE_TILE - 1u) / RG_SAMPLE_TILE; }

// Tiles of a band of `rows` output rows (only those that hold a sample row of the band).
RG_ST_HD uint32_t rg_sample_tile_count(uint32_t W, uint32_t rows, uint32_t k) {
    return rg_sample_tiles_x(W, k) * ((k * rows + RG_SAMPLE_TILE - 1u) / RG_SAMPLE_TILE);
}

// The output pixels whose samples tile `tile` (< rg_sample_tile_count) holds.
RG_ST_HD rg_px_rect rg_sample_tile_pixels(uint32_t tile, uint32_t W, uint32_t rows, uint32_t k) {
    const uint32_t tiles_x = rg_sample_tiles_x(W, k);
    const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const uint32_t sx0 = tx * RG_SAMPLE_TILE, sy0 = ty * RG_SAMPLE_TILE;
    const uint32_t sx1 = sx0 + RG_SAMPLE_TILE < k * W ? sx0 + RG_SAMPLE_TILE : k * W;        // exclusive
    const uint32_t sy1 = sy0 + RG_SAMPLE_TILE < k * rows ? sy0 + RG_SAMPLE_TILE : k * rows;  // exclusive
    return {sx0 / k, (sx1 - 1u) / k + 1u, sy0 / k, (sy1 - 1u) / k + 1u};
}

// Is the tile listed, i.e. is some pixel it overlaps flagged?  `mask`: the band's first row, W
// bytes per row.
RG_ST_HD bool rg_sample_tile_listed(const uint8_t *mask, uint32_t tile, uint32_t W, uint32_t rows, uint32_t k) {
    const rg_px_rect r = rg_sample_tile_pixels(tile, W, rows, k);
    for (uint32_t y = r.y0; y < r.y1; ++y)
        for (uint32_t x = r.x0; x < r.x1; ++x)
            if (mask[(size_t)y * W + x]) return true;
    return false;
}
