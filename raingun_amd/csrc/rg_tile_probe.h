// rg_tile_probe.h — what the two tile probes share (rg_tile_order.hip: the reference's view;
// rg_tile_order_camera.hip: a camera's): the samples per tile, a sample's weight, a tile's bucket.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/raingun.h"
#include "rg_device.h"
#include "rg_k_frames.h"
#include "rg_k_trace.h"

#pragma clang fp contract(off)

using namespace rgk;

#define RG_PROBE_SAMPLES 8   // per tile: 4 corners + 4 inner points; 8 tiles per wave
#define RG_ORDER_BUCKETS 16

__device__ __forceinline__ uint32_t probe_weight(const RgKernelArgs &a, const Closest &c) {
    if (c.id < 0) return 1u;                                        // sky: one ray
    const int s = a.mats[c.id].surface;
    const uint32_t diffuse = 2u + (uint32_t)a.n_lights;              // primary + shadow rays
    if (a.max_depth <= 1) return diffuse;
    if (s == RG_SURFACE_REFRACTIVE) return 8u * diffuse;            // a ray tree below the hit
    if (s == RG_SURFACE_REFLECTING) return 3u * diffuse;            // a reflection chain
    return diffuse;
}
// bucket 0 = heaviest; a tile's weight is the sum of its 8 samples
__device__ __forceinline__ uint32_t order_bucket(uint32_t w) {
    return (RG_ORDER_BUCKETS - 1u) - min(w >> 4, RG_ORDER_BUCKETS - 1u);
}
