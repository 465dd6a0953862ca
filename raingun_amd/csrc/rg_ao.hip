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
    dim3 grid;
    size_t lds = 0;
    const hipError_t e = rg_pass_grid(*a, RG_AO_BLOCK, RG_AO_BLOCKS_PER_CU, &grid, &lds);
    if (e != hipSuccess) return e;
    return a->camera ? launch_flavour<true>(a, o, grid, lds, stream) : launch_flavour<false>(a, o, grid, lds, stream);
}

// ---------------------------------------------------------------- host side
namespace {

bool ao_ok(const rg_ao *ao) { return ao && rg_ao_valid(ao->samples, ao->radius, ao->bias); }

hipError_t launch_pass(const RgKernelArgs *a, const void *o, hipStream_t stream) {
    return rg_launch_ao(a, static_cast<const RgAoArgs *>(o), stream);
}

// The scene's AO table on its device, made on the first AO frame.
rg_status ao_table(const rg_scene *s) {
    if (s->d_ao) return RG_OK;
    double table[RG_AO_TABLE_DOUBLES];
    rg_ao_make_table(table);
    return rg_table_once(s, s->d_ao, table, sizeof table);
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
    if (!s || !ao_ok(ao) || !ao_dev) return RG_ERR_INVALID_ARGUMENT;
    uint32_t rows = 0;
    rg_status st = rg_pass_check(s, width, height, tiling, &rows);
    if (st != RG_OK || (st = ao_table(s)) != RG_OK) return st;
    const RgAoArgs o{ao_dev, s->d_ao, ao->samples, 0u, ao->radius, ao->bias};
    return rg_pass_enqueue(s, width, height, *tiling, rows, static_cast<hipStream_t>(stream), RG_AO_TILE_WLOG, stats,
                           launch_pass, &o);
}

rg_status rg_render_ao(const rg_scene *s, uint32_t width, uint32_t height, const rg_ao *ao, float *ao_out,
                       rg_stats *stats) {
    if (!s || !ao_ok(ao) || !ao_out || width == 0 || height == 0) return RG_ERR_INVALID_ARGUMENT;
    if (width < height) return RG_ERR_PORTRAIT;
    const unsigned long long npx = (unsigned long long)width * height;
    if (npx >= (1ull << 32)) return RG_ERR_INVALID_ARGUMENT;
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    rg_scratch mem;
    float *d = mem.dev<float>((size_t)npx * sizeof(float));
    if (mem.status() != RG_OK) return mem.status();
    const rg_tiling whole = {height, 1, 0};
    rg_stats local;
    rg_status st = rg_render_ao_async(s, width, height, &whole, ao, d, nullptr, stats ? stats : &local);
    // the frame is delivered on the reference's panics too
    if (rg_delivers_frame(st) && !ok(hipMemcpy(ao_out, d, (size_t)npx * sizeof(float), hipMemcpyDeviceToHost)))
        st = RG_ERR_DEVICE;
    return st;
}

}  // extern "C"
