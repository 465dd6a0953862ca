// rg_edge.hip — the two kernels between the 1-sample pass and the sparse sample launches
// of adaptive anti-aliasing (rg_render_image_aa_adaptive / rg_render_aa_adaptive /
// rg_edge_mask, rg_aa.hip).  raingun_amd/aa.py restates the mask in numpy (edge_mask) and
// the tests compare byte for byte.
//
// 1. rg_edge_mask_kernel: flag(p) = max over c in {R, G, B} and over the up to eight
//    neighbours q of p inside the frame of |rgba[p][c] - rgba[q][c]| >= T, integers
//    throughout, alpha ignored.  A streaming 3 x 3 stencil over packed RGBA8: a block of
//    64 x 4 threads makes 256 x 4 pixels (a thread four adjacent pixels of one row) from an
//    LDS copy of its 4 rows + one halo row above and below, 256 + 2 x 4 pixels wide (the
//    halo column comes with its whole 16-B group).  VEC (rows a multiple of 16 B and the
//    buffers aligned): the copy is made with 16-B loads and a thread's four mask bytes go
//    out as one dword; else dword loads and byte stores.  Every input pixel is read from
//    memory 1.5 times (6 rows for 4) and 1 + 8/256 times across.  The flagged count: a
//    ballot per pixel of the thread, popcounts added per wave, one atomic per wave, on one of
//    RG_EDGE_SHARDS counters (a line each) that the host adds up.
// 2. rg_tile_list_kernel: per band of the plan, one thread per 8 x 8 sample tile of the
//    band's launch (rg_sample_tiles.h); a tile is listed if a pixel it overlaps is flagged.
//    Listed tiles are appended to the band's list by a wave ballot and one atomic per wave;
//    the order within a list only schedules.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "rg_launchers.h"
#include "rg_sample_tiles.h"

#define RG_EDGE_PX 4   // adjacent pixels per thread
#define RG_EDGE_BX 64  // threads across (one wave: 256 pixels)
#define RG_EDGE_BY 4   // rows per block
#define RG_EDGE_TW (RG_EDGE_PX * RG_EDGE_BX + 8)  // LDS row: the block's pixels + a 4-pixel group each side

namespace {

struct RgEdgeArgs {
    const uint32_t *rgba;  // H x W packed RGBA8
    uint8_t *mask;         // H x W
    uint32_t *flagged;     // RG_EDGE_SHARDS counters, RG_EDGE_SHARD_WORDS apart: their sum += the number of ones
    uint32_t W, H, T;
    uint32_t nbx;          // 256-pixel column blocks of a row
};

// max over R, G, B of |a - b|
__device__ __forceinline__ uint32_t rgb_contrast(uint32_t a, uint32_t b) {
    uint32_t m = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int d = (int)((a >> (8 * c)) & 0xFFu) - (int)((b >> (8 * c)) & 0xFFu);
        m = max(m, (uint32_t)(d < 0 ? -d : d));
    }
    return m;
}

template <bool VEC>
__global__ __launch_bounds__(RG_EDGE_BX *RG_EDGE_BY) void rg_edge_mask_kernel(RgEdgeArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[RG_EDGE_BY + 2][RG_EDGE_TW];
    const uint32_t tid = threadIdx.y * RG_EDGE_BX + threadIdx.x;
    const long long y0 = (long long)blockIdx.x * RG_EDGE_BY;
    uint32_t wave_ones = 0;  // wave-uniform
    for (uint32_t bx = blockIdx.y; bx < a.nbx; bx += gridDim.y) {
        const long long gx0 = (long long)bx * (RG_EDGE_PX * RG_EDGE_BX) - 4;  // frame column of tile column 0
        if (VEC) {
            constexpr uint32_t G = RG_EDGE_TW / 4;
            for (uint32_t g = tid; g < (RG_EDGE_BY + 2) * G; g += RG_EDGE_BX * RG_EDGE_BY) {
                const uint32_t r = g / G, c = g - r * G;
                const long long y = y0 + r - 1, x = gx0 + 4 * c;
                if (y >= 0 && y < (long long)a.H && x >= 0 && x < (long long)a.W)  // W % 4 == 0: the whole group
                    *reinterpret_cast<uint4 *>(&tile[r][4 * c]) =
                        *reinterpret_cast<const uint4 *>(a.rgba + (size_t)y * a.W + (size_t)x);
            }
        } else {
            for (uint32_t g = tid; g < (RG_EDGE_BY + 2) * RG_EDGE_TW; g += RG_EDGE_BX * RG_EDGE_BY) {
                const uint32_t r = g / RG_EDGE_TW, c = g - r * RG_EDGE_TW;
                const long long y = y0 + r - 1, x = gx0 + c;
                if (y >= 0 && y < (long long)a.H && x >= 0 && x < (long long)a.W)
                    tile[r][c] = a.rgba[(size_t)y * a.W + (size_t)x];
            }
        }
        __syncthreads();
        const long long y = y0 + threadIdx.y;
        const long long x = (long long)bx * (RG_EDGE_PX * RG_EDGE_BX) + threadIdx.x * RG_EDGE_PX;
        uint32_t bits = 0;  // the thread's four mask bytes
#pragma unroll
        for (int p = 0; p < RG_EDGE_PX; ++p) {
            bool flag = false;
            if (y < (long long)a.H && x + p < (long long)a.W) {
                const uint32_t tr = threadIdx.y + 1, tc = 4 + threadIdx.x * RG_EDGE_PX + p;
                const uint32_t me = tile[tr][tc];
                uint32_t m = 0;  // 0 for a pixel without neighbours
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (dy == 0 && dx == 0) continue;
                        const long long ny = y + dy, nx = x + p + dx;
                        if (ny >= 0 && ny < (long long)a.H && nx >= 0 && nx < (long long)a.W)
                            m = max(m, rgb_contrast(me, tile[tr + dy][tc + dx]));
                    }
                flag = m >= a.T;
                bits |= (flag ? 1u : 0u) << (8 * p);
            }
            wave_ones += (uint32_t)__builtin_popcountll(__ballot(flag));
        }
        if (y < (long long)a.H && x < (long long)a.W) {
            uint8_t *o = a.mask + (size_t)y * a.W + (size_t)x;
            if (VEC) {
                *reinterpret_cast<uint32_t *>(o) = bits;
            } else {
#pragma unroll
                for (int p = 0; p < RG_EDGE_PX; ++p)
                    if (x + p < (long long)a.W) o[p] = (uint8_t)((bits >> (8 * p)) & 1u);
            }
        }
        __syncthreads();  // the tile is restaged for the next column block
    }
    if (threadIdx.x == 0 && wave_ones)  // blockDim.x == 64: lane 0 of each wave
        atomicAdd(a.flagged + ((blockIdx.x * RG_EDGE_BY + threadIdx.y) % RG_EDGE_SHARDS) * RG_EDGE_SHARD_WORDS, wave_ones);
}

struct RgTileListArgs {
    const uint8_t *mask;  // H x W
    uint32_t *list;       // band b's list at list[b * stride ..]
    uint32_t *counts;     // per band, += its listed tiles
    uint32_t W, H, k, band_rows, stride;
};

__global__ __launch_bounds__(256) void rg_tile_list_kernel(RgTileListArgs a) {
    const uint32_t b = blockIdx.y, t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t r0 = b * a.band_rows;
    const uint32_t rows = min(a.H, r0 + a.band_rows) - r0;  // the last band is partial
    const bool listed = t < rg_sample_tile_count(a.W, rows, a.k) &&
                        rg_sample_tile_listed(a.mask + (size_t)r0 * a.W, t, a.W, rows, a.k);
    const unsigned long long vote = __ballot(listed);
    if (vote == 0ull) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t base = 0;
    if (lane == (uint32_t)__builtin_ctzll(vote)) base = atomicAdd(&a.counts[b], (uint32_t)__builtin_popcountll(vote));
    base = (uint32_t)__shfl((int)base, __builtin_ctzll(vote), 64);
    if (listed) {
        const uint32_t before = (uint32_t)__builtin_popcountll(vote & ((1ull << lane) - 1ull));
        a.list[(size_t)b * a.stride + base + before] = t;
    }
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" hipError_t rg_launch_edge_mask(const uint8_t *rgba, uint32_t width, uint32_t height, uint32_t threshold,
                                          uint8_t *mask, uint32_t *flagged, hipStream_t stream) {
    if (!rgba || !mask || !flagged || width == 0 || height == 0) return hipErrorInvalidValue;
    RgEdgeArgs a;
    a.rgba = reinterpret_cast<const uint32_t *>(rgba);
    a.mask = mask;
    a.flagged = flagged;
    a.W = width;
    a.H = height;
    a.T = threshold;
    a.nbx = (width + RG_EDGE_PX * RG_EDGE_BX - 1) / (RG_EDGE_PX * RG_EDGE_BX);
    const dim3 grid((height + RG_EDGE_BY - 1) / RG_EDGE_BY, std::min(a.nbx, 65535u)), block(RG_EDGE_BX, RG_EDGE_BY);
    if (width % 4 == 0 && aligned16(rgba) && (reinterpret_cast<uintptr_t>(mask) & 3u) == 0)
        hipLaunchKernelGGL(rg_edge_mask_kernel<true>, grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL(rg_edge_mask_kernel<false>, grid, block, 0, stream, a);
    return hipGetLastError();
}

extern "C" hipError_t rg_launch_tile_list(const uint8_t *mask, uint32_t width, uint32_t height, uint32_t k,
                                          uint32_t band_rows, uint32_t bands, uint32_t *list, uint32_t stride,
                                          uint32_t *counts, hipStream_t stream) {
    if (!mask || !list || !counts || width == 0 || height == 0 || k < 1 || band_rows == 0 || bands == 0 || bands > 65535u)
        return hipErrorInvalidValue;
    const uint32_t per_band = rg_sample_tile_count(width, std::min(band_rows, height), k);
    if (per_band > stride) return hipErrorInvalidValue;
    const RgTileListArgs a{mask, list, counts, width, height, k, band_rows, stride};
    hipLaunchKernelGGL(rg_tile_list_kernel, dim3((per_band + 255u) / 256u, bands), dim3(256), 0, stream, a);
    return hipGetLastError();
}
