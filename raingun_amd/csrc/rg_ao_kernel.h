// rg_ao_kernel.h — rg_ao_kernel: one pixel per lane; its primary ray, then the k x k
// any-hit rays of rg_ao.h over the hemisphere above the primary hit, the open share written as one float.
// Included by rg_ao.hip alone (its launcher and the entry points of the C ABI), the way rg_aov_kernel.h is
// by rg_aov.hip: the kernel headers it needs come with it.
#pragma once
#include <hip/hip_runtime.h>

#include "rg_ao.h"
#include "rg_camera.h"
#include "rg_device.h"
#include "rg_k_frames.h"
#include "rg_k_shade.h"
#include "rg_k_trace.h"
#include "rg_launchers.h"

#pragma clang fp contract(off)

using namespace rgk;

#define RG_AO_BLOCK 256

// AO rays leave one point in k^2 directions spread over a hemisphere: 64 lanes, 64 hit points, no two rays
// alike.  1: they walk the BVH per lane wherever the scene has the per-lane stacks (lane_stack > 0); 0: per
// lane only where rays of depth 0 do (lane_min_depth <= 0), else with the wave.  North star, k = 4 at 4K, per
// lane / with the wave: +inf 4.90 / 4.73 ms, radius 16 8.26 / 8.43 ms -- with no limit most rays end at their
// first occluder and the shared walk's wide loads win, with one they walk on and the union of 64 paths costs
// more than it shares.  Within 3 % either way; per lane, for the case that costs more (profiles/ao/ab_walk.json).
#ifndef RG_AO_LANE_WALK
#define RG_AO_LANE_WALK 1
#endif

// CAMERA, F32F, BVH: as rg_aov_kernel's.  o: the pass by value (RgAoArgs, rg_launchers.h).
template <bool CAMERA, bool F32F, bool BVH>
__global__ __launch_bounds__(RG_AO_BLOCK) void rg_ao_kernel(RgKernelArgs a, RgAoArgs o) {
    // the launch context's other counter set starts the next launch at zero (rg_internal.h rg_launch_ctx)
    if (blockIdx.x == 0 && a.counters_next)
        for (uint32_t k = threadIdx.x; k < RG_COUNTER_WORDS; k += RG_AO_BLOCK) a.counters_next[k] = 0ull;
    __shared__ unsigned long long block_prim, block_shadow;
    if (threadIdx.x == 0) {
        block_prim = 0ull;
        block_shadow = 0ull;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t twlog = a.tile_wlog, twmask = (1u << twlog) - 1u, th = 64u >> twlog;
    const uint32_t tiles_x = (a.width + twmask) >> twlog;
    const uint32_t ntiles = tiles_x * ((a.out_rows + th - 1u) / th);
    const uint32_t nwaves = gridDim.x * (RG_AO_BLOCK / 64u);
    const SphScalar src{rg_cptr(a.sph), rg_cptr(a.sph_cc), rg_cptr(a.sphf), rg_cptr(a.sphf2),
                        rg_cptr(a.pln), rg_cptr(a.dsk), rg_cptr(a.box), rg_cptr(a.nodes), a.lbuf, a.lights};
    // the pass's points and the 64 turns: wave-uniform addresses in constant memory, so scalar loads
    const uint32_t k2 = o.samples * o.samples;
    const auto *points = rg_cptr(o.tab) + 3u * rg_lens_points_offset(o.samples);
    const auto *rotations = rg_cptr(o.tab) + RG_AO_POINT_DOUBLES;
    const float den = (float)k2;
    uint32_t n_prim = 0, n_shadow = 0;
    for (uint32_t tile = blockIdx.x * (RG_AO_BLOCK / 64u) + (threadIdx.x >> 6); tile < ntiles; tile += nwaves) {
        const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const uint32_t x = (tx << twlog) + (lane & twmask);
        const uint32_t orow = ty * th + (lane >> twlog);
        const bool inside = x < a.width && orow < a.out_rows;
        const uint32_t y = inside ? out_row_to_y(a, orow) : 0u;
        const size_t oidx = (size_t)orow * a.width + x;
        const bool live = inside && y != 0xFFFFFFFFu;
        const uint32_t pixel = y * a.width + x;
        bool hit = false, erred = false;  // erred: the pixel's first error is the one reported
        double O[3] = {0.0, 0.0, 0.0}, nf[3] = {0.0, 0.0, 0.0}, Tr[3] = {0.0, 0.0, 0.0}, Br[3] = {0.0, 0.0, 0.0};
        if (live) {
            double sx, sy;
            sensor_div(a, x, y, sx, sy);  // ray.rs:43-51
            Ray r;
            Closest c;
            closest_init(c);
            n_prim++;
            if constexpr (CAMERA) {
                double dir[3];
                rg_camera_direction(a.cam_right, a.cam_up, a.cam_forward, sx, sy, dir);
                r.o = v3(a.cam_eye[0], a.cam_eye[1], a.cam_eye[2]);
                r.d = v3(dir[0], dir[1], dir[2]);
                bool occl = false;
                // a ray of depth 0: it walks per lane only where rays of every depth do
                trace_query<F32F, BVH>(a, src, r, false, 0.0, c, occl, a.lane_min_depth <= 0);
            } else {
                r.o = v3(0.0, 0.0, 0.0);
                r.d = normalize(v3(sx, sy, -1.0));
                trace_primary<F32F, BVH>(a, src, r.d, c);
            }
            if (c.nan && c.nhit >= 2) {
                raise_error(a, pixel, RG_ERR_NAN_DISTANCE);
                erred = true;
            }
            hit = c.id >= 0;
            if (hit) {
                const RgBodyDev b = a.bodies[c.id];
                const V3 hp = add(r.o, scl(r.d, c.t));  // rendering.rs get_color
                V3 n;
                if (!surface_normal(b, hp, n) && !erred) {  // (n = 1,0,0 as in get_color)
                    raise_error(a, pixel, RG_ERR_AABB_NORMAL);
                    erred = true;
                }
                const double h3[3] = {hp.x, hp.y, hp.z}, n3[3] = {n.x, n.y, n.z}, d3[3] = {r.d.x, r.d.y, r.d.z};
                double T[3], B[3];
                rg_ao_facing(n3, d3, nf);
                rg_ao_origin(h3, nf, o.bias, O);
                rg_ao_frame(nf, T, B);
                const uint32_t m = rg_ao_turn_index(pixel);
                rg_ao_turn(T, B, rotations[2u * m], rotations[2u * m + 1u], Tr, Br);
            }
        }
        uint32_t open = 0;
        if (__any(hit)) {
            for (uint32_t j = 0; j < k2; ++j) {
                const double px = points[3u * j], py = points[3u * j + 1u], pz = points[3u * j + 2u];
                if (hit) {
                    double dir[3];
                    rg_ao_direction(Tr, Br, nf, px, py, pz, dir);
                    Ray q;
                    q.o = v3(O[0], O[1], O[2]);
                    q.d = v3(dir[0], dir[1], dir[2]);
                    // a ray that could see a NaN distance (ray_exotic) runs as a fully counted closest-hit
                    // query: occluded = some hit && !(dist > radius) (rendering.rs:150-155), the scene.rs:38
                    // panic iff >= 2 hits, one NaN -- as rg_render_kernel treats such a shadow ray
                    const bool exact = a.nan_scene || ray_exotic(q.o, q.d);
                    const bool lane_walk = RG_AO_LANE_WALK ? true : a.lane_min_depth <= 0;
                    Closest c;
                    closest_init(c);
                    bool occl = false;
                    n_shadow++;
                    trace_query<F32F, BVH>(a, src, q, !exact, o.radius, c, occl, lane_walk, -1);
                    if (exact) {
                        occl = c.id >= 0 && !(c.t > o.radius);
                        if (c.nan && c.nhit >= 2 && !erred) {
                            raise_error(a, pixel, RG_ERR_NAN_DISTANCE);
                            erred = true;
                        }
                    }
                    open += occl ? 0u : 1u;
                }
            }
        }
        if (inside) o.out[oidx] = !live ? 0.0f : hit ? (float)open / den : 1.0f;
    }
    // ray counters: wave reduction, block reduction in LDS, one atomic per block and class
    const unsigned long long p64 = wave_sum(n_prim), s64 = wave_sum(n_shadow);
    if (lane == 0 && p64) atomicAdd(&block_prim, p64);
    if (lane == 0 && s64) atomicAdd(&block_shadow, s64);
    __syncthreads();
    if (threadIdx.x == 0 && block_prim) atomicAdd(&a.counters[0], block_prim);
    if (threadIdx.x == 0 && block_shadow) atomicAdd(&a.counters[1], block_shadow);
}
