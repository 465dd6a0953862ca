// rg_ao.hip — the ambient occlusion pass: how much of the hemisphere above each pixel's
// primary hit is open.  rg_ao_kernel traces the primary ray of every pixel of a tiled launch -- the ray
// rg_render_aov traces for that pixel -- and from its hit the k x k any-hit rays of rg_ao.h, each through the
// query rg_render_kernel's shadow rays take (rg_k_trace.h trace_query).  The kernel, its launcher and the
// entry points of the C ABI (rg_ao_tables / rg_render_ao / rg_render_ao_async) live in this translation unit
// alone (the kernel's text: rg_ao_kernel.h), so that every other kernel keeps the device code it had
// (DESIGN.md 4, 4s).
#include <hip/hip_runtime.h>

#include "../../include/raingun.h"
#include "rg_ao_kernel.h"
#include "rg_device.h"
#include "rg_internal.h"
#include "rg_launchers.h"

#pragma clang fp contract(off)

// Lane-to-pixel mapping: a wave is one tile of 64 pixels, 2^RG_AO_TILE_WLOG wide and 64 >> it tall (3: 8x8,
// 6: 64x1).  The k^2 rays of a lane share nothing with its neighbours' but their origin's neighbourhood, so
// the squarest tile keeps the origins -- and the leaves the walks touch -- closest together.  k = 4 at 4K,
// 8x8 / 16x4 / 32x2 / 64x1: north star +inf 4.91 / 5.04 / 5.40 / 5.71 ms, radius 16 8.26 / 8.39 / 8.94 /
// 9.43 ms; test1 (no BVH) 0.95 / 0.94 / 0.96 / 0.97 ms (profiles/ao/ab_tile_shape.json).
#ifndef RG_AO_TILE_WLOG
#define RG_AO_TILE_WLOG 3
#endif
// Blocks per CU of the one-shot grid (4 waves each); a wave strides over the launch's tiles.  A tile costs
// up to 64 k^2 + 64 rays and tiles differ (a miss costs one ray), so more, smaller shares balance better than
// the AOV kernel's 16; every block ends with two atomics, which a launch of milliseconds does not notice but
// a k = 1 frame would, so not 64 for its last percent.  16 / 32 / 64: north star +inf 5.12 / 4.89 / 4.85 ms,
// radius 16 8.60 / 8.26 / 8.21 ms; test1 0.99 / 0.95 / 0.96 ms (profiles/ao/ab_grid.json).
#ifndef RG_AO_BLOCKS_PER_CU
#define RG_AO_BLOCKS_PER_CU 32
#endif

namespace {

template <bool CAMERA>
hipError_t launch_flavour(const RgKernelArgs *a, const RgAoArgs *o, dim3 grid, size_t lds, hipStream_t stream) {
    // the query flavours of rg_trace: the BVH, else the f32 pre-filter on the heavy path, else the exact loops
    if (a->n_nodes > 0)
        hipLaunchKernelGGL((rg_ao_kernel<CAMERA, true, true>), grid, dim3(RG_AO_BLOCK), lds, stream, *a, *o);
    else if (rg_heavy_path(*a))
        hipLaunchKernelGGL((rg_ao_kernel<CAMERA, true, false>), grid, dim3(RG_AO_BLOCK), lds, stream, *a, *o);
    else
        hipLaunchKernelGGL((rg_ao_kernel<CAMERA, false, false>), grid, dim3(RG_AO_BLOCK), lds, stream, *a, *o);
    return hipGetLastError();
}

}  // namespace

extern "C" hipError_t rg_launch_ao(const RgKernelArgs *a, const RgAoArgs *o, hipStream_t stream) {
    if (a->out_rows == 0 || a->width == 0 || a->tile_wlog < 3 || a->tile_wlog > 6) return hipErrorInvalidValue;
    if (!o->out || !o->tab || !rg_ao_valid(o->samples, o->radius, o->bias)) return hipErrorInvalidValue;
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    const unsigned long long ntiles = rg_tile_count(*a), per_block = RG_AO_BLOCK / 64u;
    const unsigned long long want = (ntiles + per_block - 1ull) / per_block;
    const unsigned long long cap = (unsigned long long)(cus > 0 ? cus : 1) * RG_AO_BLOCKS_PER_CU;
    const dim3 grid((unsigned)(want < cap ? want : cap));
    // per-lane walk stacks (stride = block size): lane_stack entries + the spare slot (rg_k_bvh.h bvh_lane)
    const size_t lds = a->lane_stack > 0 ? ((size_t)(a->lane_stack + 1) * 4u) * RG_AO_BLOCK : 0u;
    return a->camera ? launch_flavour<true>(a, o, grid, lds, stream) : launch_flavour<false>(a, o, grid, lds, stream);
}

// ---------------------------------------------------------------- host side
namespace {

bool ao_ok(const rg_ao *ao) { return ao && rg_ao_valid(ao->samples, ao->radius, ao->bias); }

// The scene's arguments plus this launch's frame, tiling, camera and counter sets (what
// rg_launch_tiles sets of them; the kernel reads nothing else).
RgKernelArgs ao_args(const rg_scene *s, rg_launch_ctx *cx, uint32_t W, uint32_t H, const rg_tiling &t, uint32_t rows) {
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
    a.tile_wlog = RG_AO_TILE_WLOG;
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

// The scene's AO table on its device: made on the first AO frame, never rewritten, so launches in flight may
// read it whatever comes next.
rg_status ao_table(const rg_scene *s) {
    if (s->d_ao) return RG_OK;
    double table[RG_AO_TABLE_DOUBLES];
    rg_ao_make_table(table);
    void *d = nullptr;
    if (!ok(hipMalloc(&d, sizeof table))) {
        (void)hipGetLastError();
        return RG_ERR_OUT_OF_MEMORY;
    }
    if (!ok(hipMemcpy(d, table, sizeof table, hipMemcpyHostToDevice))) {
        (void)hipFree(d);
        return RG_ERR_DEVICE;
    }
    s->d_ao = static_cast<double *>(d);
    return RG_OK;
}

}  // namespace

extern "C" {

rg_status rg_ao_tables(uint32_t samples, double *points) {
    if (samples < 1 || samples > RG_AO_MAX_SAMPLES || !points) return RG_ERR_INVALID_ARGUMENT;
    rg_ao_make_points(samples, points);
    return RG_OK;
}

rg_status rg_render_ao_async(const rg_scene *s, uint32_t width, uint32_t height, const rg_tiling *tiling, const rg_ao *ao,
                             float *ao_dev, void *stream, rg_stats *stats) {
    if (!s || !ao_ok(ao) || !ao_dev || width == 0 || height == 0 || !tiling || !rg_tiling_valid(tiling))
        return RG_ERR_INVALID_ARGUMENT;
    if (width < height) return RG_ERR_PORTRAIT;  // ray.rs:42
    const uint32_t rows = rg_tiling_rows(height, tiling);
    if ((unsigned long long)rows * width >= (1ull << 32) || (unsigned long long)height * width >= (1ull << 32))
        return RG_ERR_INVALID_ARGUMENT;  // the reference's u32 pixel index (rendering.rs:27)
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    rg_status st = ao_table(s);
    if (st != RG_OK) return st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    rg_launch_ctx *cx = rg_ctx_for(s, hs);
    if (!cx) return RG_ERR_OUT_OF_MEMORY;
    s->last = cx;
    RgKernelArgs a = ao_args(s, cx, width, height, *tiling, rows);
    const RgAoArgs o{ao_dev, s->d_ao, ao->samples, 0u, ao->radius, ao->bias};
    cx->last_counters = a.counters;
    cx->last_plain = 0;
    cx->last_shvol = 0;
    if (stats && !ok(hipEventRecord(cx->ev0, hs))) return RG_ERR_DEVICE;
    if (rows > 0) {
        if (!ok(rg_launch_ao(&a, &o, hs))) return RG_ERR_DEVICE;
        cx->cur = 1 - cx->cur;  // the kernel zeroes the other set for the next launch
    }
    if (!stats) return RG_OK;
    unsigned long long c[4];
    if (!ok(hipEventRecord(cx->ev1, hs)) ||
        !ok(hipMemcpyAsync(c, a.counters, sizeof c, hipMemcpyDeviceToHost, hs)) || !ok(hipStreamSynchronize(hs)))
        return RG_ERR_DEVICE;
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, cx->ev0, cx->ev1);
    stats->kernel_ms = ms;
    return rg_snap_status(c, stats);
}

rg_status rg_render_ao(const rg_scene *s, uint32_t width, uint32_t height, const rg_ao *ao, float *ao_out,
                       rg_stats *stats) {
    if (!s || !ao_ok(ao) || !ao_out || width == 0 || height == 0) return RG_ERR_INVALID_ARGUMENT;
    if (width < height) return RG_ERR_PORTRAIT;
    const unsigned long long npx = (unsigned long long)width * height;
    if (npx >= (1ull << 32)) return RG_ERR_INVALID_ARGUMENT;
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    void *d = nullptr;
    if (!ok(hipMalloc(&d, (size_t)npx * sizeof(float)))) {
        (void)hipGetLastError();
        return RG_ERR_OUT_OF_MEMORY;
    }
    const rg_tiling whole = {height, 1, 0};
    rg_stats local;
    rg_status st = rg_render_ao_async(s, width, height, &whole, ao, static_cast<float *>(d), nullptr, stats ? stats : &local);
    // the frame is delivered on the reference's panics too
    if ((st == RG_OK || st == RG_ERR_AABB_NORMAL || st == RG_ERR_NAN_DISTANCE) &&
        !ok(hipMemcpy(ao_out, d, (size_t)npx * sizeof(float), hipMemcpyDeviceToHost)))
        st = RG_ERR_DEVICE;
    (void)hipFree(d);
    return st;
}

}  // extern "C"
