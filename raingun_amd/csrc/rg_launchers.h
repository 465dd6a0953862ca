// rg_launchers.h — the launchers rg_kernels.hip, rg_tile_order.hip, rg_tile_order_camera.hip, rg_resolve.hip, rg_edge.hip,
// rg_aov.hip and rg_ao.hip define for the host side (rg_launch.hip, rg_capi.hip, rg_aa.hip).  The defining files
// include this header too, so the compiler checks every signature against it.
#pragma once
#include <hip/hip_runtime.h>

#include "rg_device.h"

// plain (nullable): set to 1 when the launch runs a PLAIN light instantiation (rg_render_launch.h), else to 0
extern "C" hipError_t rg_launch_render(const RgKernelArgs *a, int maxd, hipStream_t stream, int *plain);
extern "C" int rg_host_array_frames(void);
extern "C" hipError_t rg_render_grid_threads(const RgKernelArgs *a, int maxd, size_t *threads);
extern "C" int rg_max_array_frames(void);
extern "C" int rg_launch_global_frames(const RgKernelArgs *a, int maxd);
extern "C" hipError_t rg_launch_tile_order(const RgKernelArgs *a, uint32_t *scratch, uint32_t *perm, hipStream_t stream);
extern "C" size_t rg_tile_order_scratch_words(uint32_t ntiles);
// rg_tile_order_camera.hip: rg_launch_tile_order's probe for a launch with a camera (a->camera != 0)
extern "C" hipError_t rg_launch_tile_probe_camera(const RgKernelArgs *a, uint32_t *bucket_of, uint32_t ntiles,
                                                  hipStream_t stream);
// rg_resolve.hip: rows x width output pixels from (k rows) x (k width) packed f32 RGB samples
// (device memory; rgb nullable); hipErrorInvalidValue for k outside 1..8.
extern "C" hipError_t rg_launch_resolve(const float *in, uint32_t width, uint32_t rows, uint32_t k, uint8_t *rgba,
                                        float *rgb, hipStream_t stream);
extern "C" hipError_t rg_launch_trace(const RgKernelArgs *a, const double *rays, uint32_t n, double *dist,
                                      int32_t *body, hipStream_t stream);
// rg_aov.hip: the AOV layers of the launch's pixels (rg_aov of include/raingun.h as device pointers, each
// nullable; packing of a->rgba's rows).  Reads of `a` the scene's tables, the frame, tiling and camera
// members, tile_wlog (the wave's tile shape) and the counter sets; primary rays count into a->counters[0].
struct RgAovOut {
    int32_t *body;
    double *depth;
    float *normal, *uv, *albedo;
};
extern "C" hipError_t rg_launch_aov(const RgKernelArgs *a, const RgAovOut *o, hipStream_t stream);
// rg_ao.hip: the ambient occlusion of the launch's pixels (rg_ao of include/raingun.h by value; rg_ao.h).  out:
// a->out_rows x a->width floats (device), packed as a->rgba's rows; tab: the scene's device table
// (RG_AO_TABLE_DOUBLES doubles).  Reads of `a` what rg_launch_aov reads; primary rays count into
// a->counters[0], AO rays into a->counters[1].
struct RgAoArgs {
    float *out;
    const double *tab;
    uint32_t samples, _pad;
    double radius, bias;
};
extern "C" hipError_t rg_launch_ao(const RgKernelArgs *a, const RgAoArgs *o, hipStream_t stream);
// rg_ao_filter.hip: the edge-stopping filter of the AO pass (rg_ao_filter of include/raingun.h; rg_ambient.h) over
// a width x height frame in device memory: ao, body, out one element per pixel, normal three; out may not alias
// ao.  hipErrorInvalidValue for a null pointer, a zero size, radius outside 1 .. 8 or normal_min outside [0, 1].
extern "C" hipError_t rg_launch_ao_filter(const float *ao, const int32_t *body, const float *normal, uint32_t width,
                                          uint32_t height, uint32_t radius, float normal_min, float *out,
                                          hipStream_t stream);
// rg_ao_filter.hip: the ambient term added to npx pixels (rg_render_image_ambient's compose): rgb, albedo three
// floats per pixel, body, aof one; share: n_share floats, one per body (a body id outside the table composes as a
// miss); rgba npx RGBA8 pixels; rgb_out (nullable, may be rgb): the clamped sums.
extern "C" hipError_t rg_launch_ambient_compose(const float *rgb, const float *albedo, const int32_t *body,
                                                const float *aof, const float *share, uint32_t n_share,
                                                const float color[3], unsigned long long npx, uint8_t *rgba,
                                                float *rgb_out, hipStream_t stream);
// rg_kernels.hip: *bad (device, zeroed by the caller) += the pixels of the a->width x a->height frame whose
// camera direction differs between the general and the PLAIN kernels' arithmetic (rg_debug_camera_check).
extern "C" hipError_t rg_launch_camera_check(const RgKernelArgs *a, unsigned long long *bad, hipStream_t stream);
// *bad (zeroed by the caller) += the operands a[i] (and b[i], op 2) for which the PLAIN kernels' guarded
// sqrt / reciprocal / division differs from the compiler's in any bit (rg_debug_unscaled_check).
// out: scratch for 2 n doubles.
extern "C" hipError_t rg_launch_unscaled_check(int op, const double *a, const double *b, uint32_t n, double *out,
                                               unsigned long long *bad, hipStream_t stream);
// rg_resolve.hip: the resolve of adaptive anti-aliasing over rows x width output pixels: pixels
// whose mask byte is non-zero become the box resolve of their k x k samples of `in` (nullable:
// none), the others keep rgba and get their rgb (nullable) clamped in place.
extern "C" hipError_t rg_launch_resolve_adaptive(const float *in, const uint8_t *mask, uint32_t width, uint32_t rows,
                                                 uint32_t k, uint8_t *rgba, float *rgb, hipStream_t stream);
// rg_edge.hip: mask[p] = 1 where the 8-neighbourhood contrast of packed RGBA8 pixel p is >= threshold,
// else 0.  The number of ones is added to `flagged` (device, zeroed by the caller): RG_EDGE_SHARDS
// counters, RG_EDGE_SHARD_WORDS words (one 128-B line) apart, whose sum it is -- a 4K frame is 32,400
// waves, and that many atomics on one address alone take ~0.2 ms (measured: DESIGN.md 4p).
#define RG_EDGE_SHARDS 64
#define RG_EDGE_SHARD_WORDS 32
extern "C" hipError_t rg_launch_edge_mask(const uint8_t *rgba, uint32_t width, uint32_t height, uint32_t threshold,
                                          uint8_t *mask, uint32_t *flagged, hipStream_t stream);
// rg_edge.hip: for each of `bands` bands of band_rows output rows (the last partial), the 8x8 sample
// tiles of the band's k-fold launch that overlap a flagged pixel (rg_sample_tiles.h), appended to
// list[b * stride ..] with counts[b] (device, zeroed by the caller) += their number.
extern "C" hipError_t rg_launch_tile_list(const uint8_t *mask, uint32_t width, uint32_t height, uint32_t k,
                                          uint32_t band_rows, uint32_t bands, uint32_t *list, uint32_t stride,
                                          uint32_t *counts, hipStream_t stream);
