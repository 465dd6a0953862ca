// rg_gather.hip — the two kernels around a gather of parts (rg_frames.hip, rg_multi.hip's gather
// mode): pack a rendered RGBA part to RGB before it is sent, and re-interleave the gathered
// parts into the image (the deal of rg_tile_deal.h).
#include <hip/hip_runtime.h>

#include "rg_internal.h"
#include "rg_tile_deal.h"

namespace {

// The gathered parts travel as packed RGB, 3 B per pixel: alpha is always
// 255 (color.rs rgba()), so a quarter of every gather's bytes over xGMI carried
// no information.  Non-root ranks pack their part after the render; the root
// re-interleaves its OWN rows straight from its RGBA part (its slot of the
// gather is not read) and the others' from the packed slots, re-adding alpha.
__global__ __launch_bounds__(256) void rg_pack_rgb_kernel(const uint32_t *rgba, uint8_t *rgb, size_t npx) {
    const size_t g = (size_t)blockIdx.x * 256u + threadIdx.x;  // pixels 4g .. 4g+3
    const size_t p0 = g * 4u;
    if (p0 >= npx) return;
    if (p0 + 4u <= npx) {
        const uint4 v = reinterpret_cast<const uint4 *>(rgba)[g];
        uint32_t *o = reinterpret_cast<uint32_t *>(rgb + p0 * 3u);  // 12 g bytes: dword aligned
        o[0] = (v.x & 0xFFFFFFu) | (v.y << 24);
        o[1] = ((v.y >> 8) & 0xFFFFu) | (v.z << 16);
        o[2] = ((v.z >> 16) & 0xFFu) | ((v.w & 0xFFFFFFu) << 8);
    } else {
        for (size_t p = p0; p < npx; ++p) {
            const uint32_t v = rgba[p];
            rgb[3 * p] = (uint8_t)v;
            rgb[3 * p + 1] = (uint8_t)(v >> 8);
            rgb[3 * p + 2] = (uint8_t)(v >> 16);
        }
    }
}

// Image row y comes from row from.at of rank from.rank's part (rg_deal_source_row;
// distributed.py assemble).  Rank 0's rows come from root_part (RGBA), the others' from
// their packed slots (slot_bytes apart).  4 pixels per thread.
__global__ __launch_bounds__(256) void rg_reinterleave_kernel(const uint8_t *gathered, const uint32_t *root_part,
                                                              uint32_t *image, uint32_t width, uint32_t height,
                                                              uint32_t tile_rows, uint32_t world, uint32_t root,
                                                              size_t slot_bytes) {
    const uint32_t y = blockIdx.y;
    const uint32_t x0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (y >= height || x0 >= width) return;
    const rg_deal_place from = rg_deal_source_row({tile_rows, world, root}, y);
    const uint32_t r = from.rank;
    uint32_t *dst = image + (size_t)y * width + x0;
    const size_t src_px = (size_t)from.at * width + x0;
    if (r == 0) {
        const uint32_t n = min(4u, width - x0);
        for (uint32_t k = 0; k < n; ++k) dst[k] = root_part[src_px + k];
        return;
    }
    const uint8_t *src = gathered + (size_t)r * slot_bytes + src_px * 3u;
    if ((width & 3u) == 0u) {  // whole, dword-aligned groups of 4 pixels
        const uint32_t *w = reinterpret_cast<const uint32_t *>(src);
        const uint32_t a = w[0], b = w[1], c = w[2];
        uint4 o;
        o.x = (a & 0xFFFFFFu) | 0xFF000000u;
        o.y = (a >> 24) | ((b & 0xFFFFu) << 8) | 0xFF000000u;
        o.z = (b >> 16) | ((c & 0xFFu) << 16) | 0xFF000000u;
        o.w = (c >> 8) | 0xFF000000u;
        *reinterpret_cast<uint4 *>(dst) = o;
    } else {
        const uint32_t n = min(4u, width - x0);
        for (uint32_t k = 0; k < n; ++k)
            dst[k] = (uint32_t)src[3 * k] | ((uint32_t)src[3 * k + 1] << 8) | ((uint32_t)src[3 * k + 2] << 16) |
                     0xFF000000u;
    }
}

}  // namespace

hipError_t rg_launch_pack_rgb(const void *rgba, void *rgb, size_t npx, hipStream_t stream) {
    const size_t groups = (npx + 3u) / 4u;
    hipLaunchKernelGGL(rg_pack_rgb_kernel, dim3((unsigned)((groups + 255u) / 256u)), dim3(256), 0, stream,
                       static_cast<const uint32_t *>(rgba), static_cast<uint8_t *>(rgb), npx);
    return hipGetLastError();
}

hipError_t rg_launch_reinterleave(const void *gathered, const void *root_part, void *image, uint32_t width,
                                  uint32_t height, uint32_t tile_rows, uint32_t world, size_t slot_bytes,
                                  hipStream_t stream, uint32_t root) {
    dim3 grid((((width + 3u) / 4u) + 255u) / 256u, height);
    hipLaunchKernelGGL(rg_reinterleave_kernel, grid, dim3(256), 0, stream, static_cast<const uint8_t *>(gathered),
                       static_cast<const uint32_t *>(root_part), static_cast<uint32_t *>(image), width, height,
                       tile_rows, world, root, slot_bytes);
    return hipGetLastError();
}
