// rg_aov.hip — AOV layers: what lies under each pixel.  rg_aov_kernel traces the
// primary ray of every pixel of a tiled launch -- the ray rg_render_image traces for that pixel:
// create_prime, or the scene's camera -- stops at the primary hit and writes the requested layers:
// body id, distance, geometric normal, texture coordinates and unlit surface colour, the last three
// with the shading functions of rg_k_shade.h in the reference's operation order.  The kernel, its
// launcher and the two entry points of the C ABI (rg_render_aov / rg_render_aov_async) live in this
// translation unit alone (the kernel's text: rg_aov_kernel.h), so that every other kernel keeps the
// device code it had.
#include <hip/hip_runtime.h>

#include "../../include/raingun.h"
#include "rg_aov_kernel.h"
#include "rg_device.h"
#include "rg_internal.h"
#include "rg_launchers.h"

#pragma clang fp contract(off)

// Lane-to-pixel mapping: a wave is one tile of 64 pixels, 2^RG_AOV_TILE_WLOG wide and 64 >> it tall
// (3: 8x8, the render kernels' tile and the BVH walk's coherence; 6: 64 consecutive pixels of a row,
// whole cache lines per store).  32x2: a lane's stores to a 4-byte layer fill one 128-B line per tile
// row, and the wave's rays stay close enough for the walk.  All five layers at 4K, 8x8 / 16x4 / 32x2 /
// 64x1: test1 0.139 / 0.135 / 0.128 / 0.132 ms, north star 0.174 / 0.168 / 0.169 / 0.174 ms
// (profiles/aov/ab_tile_shape.json).
#ifndef RG_AOV_TILE_WLOG
#define RG_AOV_TILE_WLOG 5
#endif
// Blocks per CU of the one-shot grid (4 waves each); a wave strides over the launch's tiles.  Every
// block ends with one atomic on the primary-ray counter, and one address takes ~80 of them per
// microsecond: 64 blocks per CU (16,384 atomics) cost 0.1 ms of a 4K launch, 4 leave the dispatcher
// nothing to balance with.  4 / 8 / 16 / 64: test1 0.141 / 0.126 / 0.126 / 0.231 ms, north star
// 0.180 / 0.170 / 0.153 / 0.216 ms (profiles/aov/ab_grid.json).
#ifndef RG_AOV_BLOCKS_PER_CU
#define RG_AOV_BLOCKS_PER_CU 16
#endif

namespace {

template <bool CAMERA, bool F32F, bool BVH>
hipError_t launch_shade(const RgKernelArgs *a, const RgAovOut *o, dim3 grid, size_t lds, hipStream_t stream) {
    if (o->normal || o->uv || o->albedo)
        hipLaunchKernelGGL((rg_aov_kernel<CAMERA, F32F, BVH, true>), grid, dim3(RG_AOV_BLOCK), lds, stream, *a, *o);
    else
        hipLaunchKernelGGL((rg_aov_kernel<CAMERA, F32F, BVH, false>), grid, dim3(RG_AOV_BLOCK), lds, stream, *a, *o);
    return hipGetLastError();
}

template <bool CAMERA>
hipError_t launch_flavour(const RgKernelArgs *a, const RgAovOut *o, dim3 grid, size_t lds, hipStream_t stream) {
    // the query flavours of rg_trace: the BVH, else the f32 pre-filter on the heavy path, else the exact loops
    if (a->n_nodes > 0) return launch_shade<CAMERA, true, true>(a, o, grid, lds, stream);
    if (rg_heavy_path(*a)) return launch_shade<CAMERA, true, false>(a, o, grid, lds, stream);
    return launch_shade<CAMERA, false, false>(a, o, grid, lds, stream);
}

}  // namespace

extern "C" hipError_t rg_launch_aov(const RgKernelArgs *a, const RgAovOut *o, hipStream_t stream) {
    if (a->out_rows == 0 || a->width == 0 || a->tile_wlog < 3 || a->tile_wlog > 6) return hipErrorInvalidValue;
    dim3 grid;
    size_t lds = 0;
    const hipError_t e = rg_pass_grid(*a, RG_AOV_BLOCK, RG_AOV_BLOCKS_PER_CU, &grid, &lds);
    if (e != hipSuccess) return e;
    return a->camera ? launch_flavour<true>(a, o, grid, lds, stream) : launch_flavour<false>(a, o, grid, lds, stream);
}

// ---------------------------------------------------------------- host side
namespace {

bool any_layer(const rg_aov *v) { return v->body || v->depth || v->normal || v->uv || v->albedo; }

hipError_t launch_pass(const RgKernelArgs *a, const void *o, hipStream_t stream) {
    return rg_launch_aov(a, static_cast<const RgAovOut *>(o), stream);
}

}  // namespace

extern "C" {

rg_status rg_render_aov_async(const rg_scene *s, uint32_t width, uint32_t height, const rg_tiling *tiling,
                              const rg_aov *dev, void *stream, rg_stats *stats) {
    if (!s || !dev || !any_layer(dev)) return RG_ERR_INVALID_ARGUMENT;
    uint32_t rows = 0;
    const rg_status st = rg_pass_check(s, width, height, tiling, &rows);
    if (st != RG_OK) return st;
    const RgAovOut o{dev->body, dev->depth, dev->normal, dev->uv, dev->albedo};
    return rg_pass_enqueue(s, width, height, *tiling, rows, static_cast<hipStream_t>(stream), RG_AOV_TILE_WLOG, stats,
                           launch_pass, &o);
}

rg_status rg_render_aov(const rg_scene *s, uint32_t width, uint32_t height, const rg_aov *out, rg_stats *stats) {
    if (!s || !out || !any_layer(out) || width == 0 || height == 0) return RG_ERR_INVALID_ARGUMENT;
    if (width < height) return RG_ERR_PORTRAIT;
    const unsigned long long npx = (unsigned long long)width * height;
    if (npx >= (1ull << 32)) return RG_ERR_INVALID_ARGUMENT;
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    // the requested layers in device memory, one plain copy each after the launch
    void *const host[5] = {out->body, out->depth, out->normal, out->uv, out->albedo};
    const size_t px_bytes[5] = {4, 8, 12, 8, 12};
    rg_scratch mem;
    void *d[5];
    for (int k = 0; k < 5; ++k) d[k] = host[k] ? mem.dev<void>((size_t)npx * px_bytes[k]) : nullptr;
    if (mem.status() != RG_OK) return mem.status();
    const rg_aov dev{static_cast<int32_t *>(d[0]), static_cast<double *>(d[1]), static_cast<float *>(d[2]),
                     static_cast<float *>(d[3]), static_cast<float *>(d[4])};
    const rg_tiling whole = {height, 1, 0};
    rg_stats local;
    rg_status st = rg_render_aov_async(s, width, height, &whole, &dev, nullptr, stats ? stats : &local);
    const bool deliver = rg_delivers_frame(st);  // on the reference's panics too
    for (int k = 0; k < 5 && deliver; ++k)
        if (host[k] && !ok(hipMemcpy(host[k], d[k], (size_t)npx * px_bytes[k], hipMemcpyDeviceToHost)))
            st = RG_ERR_DEVICE;
    return st;
}

}  // extern "C"
