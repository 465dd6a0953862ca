// rg_tile_deal.h — how a frame's tile_rows-row tiles are dealt to the ranks of the N-rank frame
// loop (rg_frames.hip) and the devices of rg_render_multi (rg_multi.hip), what that makes of a
// rank's part and of the gather slots, where the re-interleave (rg_gather.hip) finds an image
// row, and how rg_render_multi's direct mode cuts a device's share into bands and copies them
// to their image rows.  Plain integer arithmetic, no HIP: tests/native/tile_deal_test.cpp checks
// it on the CPU.  raingun_amd/distributed.py states the same deal for the Python pipeline.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/raingun.h"

#ifdef __HIPCC__
#define RG_DEAL_HD __host__ __device__  // the re-interleave kernel calls these
#else
#define RG_DEAL_HD
#endif

// ---------------------------------------------------------------- tilings
inline bool rg_tiling_valid(const rg_tiling *t) {
    return t && t->tile_rows > 0 && t->tile_stride > 0 && t->tile_offset < t->tile_stride;
}

// Rows a tiling selects when its tiles come in groups of `group` consecutive image tiles per
// stride (group 1: rg_tiling_rows); 0 for an invalid tiling or group (offset + group > stride).
// The i-th selected tile is image tile
//     group > 1 ? (i / group) * stride + offset + i % group : i * stride + offset
// -- the render kernel's own statement of it is out_row_to_y (rg_k_frames.h), which the CPU
// test restates.
inline uint32_t rg_tiling_rows_grouped(uint32_t height, const rg_tiling *t, uint32_t group) {
    if (!rg_tiling_valid(t) || height == 0 || group < 1 || (group > 1 && t->tile_offset + group > t->tile_stride)) return 0;
    const uint32_t tiles = (height + t->tile_rows - 1) / t->tile_rows;
    // per stride of image tiles: tiles offset .. offset + group - 1 (group 1: the round robin)
    const uint32_t full = tiles / t->tile_stride, rem = tiles % t->tile_stride;
    const uint32_t last = rem > t->tile_offset ? std::min(group, rem - t->tile_offset) : 0u;
    return (full * group + last) * t->tile_rows;
}

// ---------------------------------------------------------------- the deal
// Tiles of T rows are dealt to `world` ranks in periods of P = root + world - 1: the first `root`
// tiles of each period to rank 0, then one to each other rank (root 1: the round robin, tile
// t -> rank t % world).  A rank's part holds its tiles densely, in image order.
struct rg_deal {
    uint32_t T, world, root;
};
struct rg_deal_place {
    uint32_t rank, at;  // a tile: its index in the rank's part; a row: its row of the part
};

inline uint32_t rg_deal_image_tiles(const rg_deal &d, uint32_t height) { return (height + d.T - 1) / d.T; }

// Owner of image tile t and t's index among the owner's tiles.
RG_DEAL_HD inline rg_deal_place rg_deal_tile(const rg_deal &d, uint32_t t) {
    const uint32_t P = d.root + d.world - 1u;
    const uint32_t p = t / P, j = t - p * P;
    const uint32_t r = j < d.root ? 0u : j - d.root + 1u;
    return {r, r == 0u ? p * d.root + j : p};
}

// Image row y: the rank whose part holds it and its row there (the re-interleave's source).
RG_DEAL_HD inline rg_deal_place rg_deal_source_row(const rg_deal &d, uint32_t y) {
    const uint32_t t = y / d.T;
    const rg_deal_place o = rg_deal_tile(d, t);
    return {o.rank, o.at * d.T + (y - t * d.T)};
}

// A rank's tiles as a launch: rank 0 takes `root` consecutive tiles per period (a grouped
// tiling), rank r > 0 tile root + r - 1 of each period.
inline rg_tiling rg_deal_tiling(const rg_deal &d, uint32_t rank) {
    return {d.T, d.root + d.world - 1u, rank == 0 ? 0u : d.root + rank - 1u};
}
inline uint32_t rg_deal_group(const rg_deal &d, uint32_t rank) { return rank == 0 ? d.root : 1u; }

// Rows of a rank's part (whole tiles: the image's last tile is padded) and its number of tiles.
inline uint32_t rg_deal_part_rows(const rg_deal &d, uint32_t height, uint32_t rank) {
    const rg_tiling t = rg_deal_tiling(d, rank);
    return rg_tiling_rows_grouped(height, &t, rg_deal_group(d, rank));
}
inline uint32_t rg_deal_rank_tiles(const rg_deal &d, uint32_t height, uint32_t rank) {
    return rg_deal_part_rows(d, height, rank) / d.T;
}

// Rows of the equal-size gather slots: the largest part that travels.  Round robin: rank 0's
// (no rank holds more, and its slot is as large as the others'); root > 1: rank 1's, which
// holds the most tiles of the ranks whose parts are sent (rank 0's larger part is not).
inline uint32_t rg_deal_slot_rows(const rg_deal &d, uint32_t height) {
    return rg_deal_part_rows(d, height, d.root == 1 || d.world == 1 ? 0u : 1u);
}

// Bytes of a gather slot: the part as packed RGB (3 B per pixel), in whole 16-B units.
inline size_t rg_packed_slot_bytes(uint32_t slot_rows, uint32_t width) {
    return ((size_t)slot_rows * width * 3u + 15u) & ~(size_t)15u;
}

// ---------------------------------------------------------------- rg_render_multi, direct mode
#ifndef RG_MULTI_BAND_PX
#define RG_MULTI_BAND_PX (1u << 20)  // a device's share is cut into bands of about this many pixels
#endif
#define RG_MULTI_MAX_BANDS 4  // bands of a device's share at most

// Bands asked for: forced > 0 (rg_debug_set_multi), else one per RG_MULTI_BAND_PX pixels of a share.
inline int rg_multi_bands(int forced, uint32_t W, uint32_t H, int n) {
    if (forced > 0) return std::min(forced, RG_MULTI_MAX_BANDS);
    const size_t share = ((size_t)W * H + (size_t)n - 1) / (size_t)n;
    return (int)std::max<size_t>(1, std::min<size_t>(RG_MULTI_MAX_BANDS, share / RG_MULTI_BAND_PX));
}

// Every device's share (round robin over n devices) in K bands of J of its tiles each; device
// 0 holds the most tiles (per_dev), so its K bands are all non-empty.
struct rg_multi_plan {
    uint32_t H, T, n, tiles, per_dev, J;
    int K;
};

inline rg_multi_plan rg_multi_band_plan(uint32_t W, uint32_t H, uint32_t T, int n, int forced) {
    rg_multi_plan p;
    p.H = H;
    p.T = T;
    p.n = (uint32_t)n;
    p.tiles = (H + T - 1) / T;
    p.per_dev = (p.tiles + p.n - 1) / p.n;
    const uint32_t bands = (uint32_t)rg_multi_bands(forced, W, H, n);
    p.J = (p.per_dev + bands - 1) / bands;
    p.K = (int)((p.per_dev + p.J - 1) / p.J);
    return p;
}

// Band b of device i: its tiles [j0, j1) of the device's part (j1 == j0: none).  Tile j of
// device i is image tile j * n + i, so the band's `full` whole tiles go to the image in one
// strided copy (tile pitch n * T rows) from row dst_row on; the image's partial last tile, if
// it is in this band, follows them in the part and goes to rows [partial_row, partial_row +
// partial_rows) on its own.
struct rg_multi_band {
    uint32_t j0, j1, full;
    bool has_partial;
    size_t dst_row, partial_row, partial_rows;
};

inline rg_multi_band rg_multi_band_of(const rg_multi_plan &p, uint32_t i, uint32_t b) {
    rg_multi_band c{};
    const uint32_t sel = p.tiles > i ? (p.tiles - i + p.n - 1) / p.n : 0u;  // tiles of device i
    c.j0 = std::min(sel, b * p.J);
    c.j1 = std::min(sel, c.j0 + p.J);
    if (c.j1 == c.j0) return c;
    const uint32_t last_j = (p.tiles - 1u - i) / p.n;  // valid: sel > 0
    c.has_partial = (p.tiles - 1u) % p.n == i && c.j1 - 1 == last_j && p.H % p.T != 0;
    c.full = (c.j1 - c.j0) - (c.has_partial ? 1u : 0u);
    c.dst_row = ((size_t)c.j0 * p.n + (size_t)i) * p.T;
    if (c.has_partial) {
        c.partial_row = (size_t)(p.tiles - 1u) * p.T;
        c.partial_rows = p.H - c.partial_row;
    }
    return c;
}

// Image rows [y0, y1) that are complete once every device has copied its band b.
struct rg_row_range {
    size_t y0, y1;
};
inline rg_row_range rg_multi_band_rows(const rg_multi_plan &p, uint32_t b) {
    const size_t rows = (size_t)p.J * p.n * p.T;
    return {std::min<size_t>(p.H, b * rows), std::min<size_t>(p.H, (b + 1) * rows)};
}
