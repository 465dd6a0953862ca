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
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    const unsigned long long ntiles = rg_tile_count(*a), per_block = RG_AOV_BLOCK / 64u;
    const unsigned long long want = (ntiles + per_block - 1ull) / per_block;
    const unsigned long long cap = (unsigned long long)(cus > 0 ? cus : 1) * RG_AOV_BLOCKS_PER_CU;
    const dim3 grid((unsigned)(want < cap ? want : cap));
    // per-lane walk stacks (stride = block size): lane_stack entries + the spare slot (rg_k_bvh.h bvh_lane)
    const size_t lds = a->lane_stack > 0 ? ((size_t)(a->lane_stack + 1) * 4u) * RG_AOV_BLOCK : 0u;
    return a->camera ? launch_flavour<true>(a, o, grid, lds, stream) : launch_flavour<false>(a, o, grid, lds, stream);
}

// ---------------------------------------------------------------- host side
namespace {

bool any_layer(const rg_aov *v) { return v->body || v->depth || v->normal || v->uv || v->albedo; }

// The scene's arguments plus this launch's frame, tiling, camera and counter sets (what
// rg_launch_tiles sets of them; the kernel reads nothing else).
RgKernelArgs aov_args(const rg_scene *s, rg_launch_ctx *cx, uint32_t W, uint32_t H, const rg_tiling &t, uint32_t rows) {
    RgKernelArgs a = rg_make_args(s);
    a.counters = cx->counters + (size_t)cx->cur * RG_COUNTER_WORDS;  // zero (rg_launch_ctx::counters)
    a.counters_next = cx->counters + (size_t)(1 - cx->cur) * RG_COUNTER_WORDS;
    a.err_sticky = cx->sticky;
    a.width = W;
    a.height = H;
    a.tile_rows = t.tile_rows;
    a.tile_stride = t.tile_stride;
    a.tile_offset = t.tile_offset;
    a.tile_group = 1u;
    a.out_rows = rows;
    a.width_d = (double)W;
    a.height_d = (double)H;
    a.aspect = a.width_d / a.height_d;
    a.tile_wlog = RG_AOV_TILE_WLOG;
    if (s->has_camera) {  // by value: this launch keeps its camera whatever the scene is given next
        a.camera = 1u;
        for (int k = 0; k < 3; ++k) {
            a.cam_eye[k] = s->camera.eye[k];
            a.cam_right[k] = s->camera.right[k];
            a.cam_up[k] = s->camera.up[k];
            a.cam_forward[k] = s->camera.forward[k];
        }
    }
    return a;
}

}  // namespace

extern "C" {

rg_status rg_render_aov_async(const rg_scene *s, uint32_t width, uint32_t height, const rg_tiling *tiling,
                              const rg_aov *dev, void *stream, rg_stats *stats) {
    if (!s || !dev || !any_layer(dev) || width == 0 || height == 0 || !tiling || !rg_tiling_valid(tiling))
        return RG_ERR_INVALID_ARGUMENT;
    if (width < height) return RG_ERR_PORTRAIT;  // ray.rs:42
    const uint32_t rows = rg_tiling_rows(height, tiling);
    if ((unsigned long long)rows * width >= (1ull << 32) || (unsigned long long)height * width >= (1ull << 32))
        return RG_ERR_INVALID_ARGUMENT;  // the reference's u32 pixel index (rendering.rs:27)
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    rg_launch_ctx *cx = rg_ctx_for(s, st);
    if (!cx) return RG_ERR_OUT_OF_MEMORY;
    s->last = cx;
    RgKernelArgs a = aov_args(s, cx, width, height, *tiling, rows);
    const RgAovOut o{dev->body, dev->depth, dev->normal, dev->uv, dev->albedo};
    cx->last_counters = a.counters;
    cx->last_plain = 0;
    cx->last_shvol = 0;
    if (stats && !ok(hipEventRecord(cx->ev0, st))) return RG_ERR_DEVICE;
    if (rows > 0) {
        if (!ok(rg_launch_aov(&a, &o, st))) return RG_ERR_DEVICE;
        cx->cur = 1 - cx->cur;  // the kernel zeroes the other set for the next launch
    }
    if (!stats) return RG_OK;
    unsigned long long c[4];
    if (!ok(hipEventRecord(cx->ev1, st)) ||
        !ok(hipMemcpyAsync(c, a.counters, sizeof c, hipMemcpyDeviceToHost, st)) || !ok(hipStreamSynchronize(st)))
        return RG_ERR_DEVICE;
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, cx->ev0, cx->ev1);
    stats->kernel_ms = ms;
    return rg_snap_status(c, stats);
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
    void *d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    rg_status st = RG_OK;
    for (int k = 0; k < 5 && st == RG_OK; ++k)
        if (host[k] && !ok(hipMalloc(&d[k], (size_t)npx * px_bytes[k]))) {
            (void)hipGetLastError();
            st = RG_ERR_OUT_OF_MEMORY;
        }
    if (st == RG_OK) {
        const rg_aov dev{static_cast<int32_t *>(d[0]), static_cast<double *>(d[1]), static_cast<float *>(d[2]),
                         static_cast<float *>(d[3]), static_cast<float *>(d[4])};
        const rg_tiling whole = {height, 1, 0};
        rg_stats local;
        st = rg_render_aov_async(s, width, height, &whole, &dev, nullptr, stats ? stats : &local);
        // the frame is delivered on the reference's panics too
        if (st == RG_OK || st == RG_ERR_AABB_NORMAL || st == RG_ERR_NAN_DISTANCE)
            for (int k = 0; k < 5; ++k)
                if (host[k] && !ok(hipMemcpy(host[k], d[k], (size_t)npx * px_bytes[k], hipMemcpyDeviceToHost)))
                    st = RG_ERR_DEVICE;
    }
    for (int k = 0; k < 5; ++k)
        if (d[k]) (void)hipFree(d[k]);
    return st;
}

}  // extern "C"
