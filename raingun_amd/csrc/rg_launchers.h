// rg_launchers.h — the launchers rg_kernels.hip, rg_tile_order.hip and rg_resolve.hip
// define for the host side (rg_launch.hip, rg_capi.hip, rg_aa.hip).  The defining files
// include this header too, so the compiler checks every signature against it.
#pragma once
#include <hip/hip_runtime.h>

#include "rg_device.h"

extern "C" hipError_t rg_launch_render(const RgKernelArgs *a, int maxd, hipStream_t stream);
extern "C" int rg_host_array_frames(void);
extern "C" hipError_t rg_render_grid_threads(const RgKernelArgs *a, int maxd, size_t *threads);
extern "C" int rg_max_array_frames(void);
extern "C" int rg_launch_global_frames(const RgKernelArgs *a, int maxd);
extern "C" hipError_t rg_launch_tile_order(const RgKernelArgs *a, uint32_t *scratch, uint32_t *perm, hipStream_t stream);
extern "C" size_t rg_tile_order_scratch_words(uint32_t ntiles);
// rg_resolve.hip: rows x width output pixels from (k rows) x (k width) packed f32 RGB samples
// (device memory; rgb nullable); hipErrorInvalidValue for k outside 1..8.
extern "C" hipError_t rg_launch_resolve(const float *in, uint32_t width, uint32_t rows, uint32_t k, uint8_t *rgba,
                                        float *rgb, hipStream_t stream);
extern "C" hipError_t rg_launch_trace(const RgKernelArgs *a, const double *rays, uint32_t n, double *dist,
                                      int32_t *body, hipStream_t stream);
