// rg_aov_kernel.h — rg_aov_kernel: one primary ray per lane, stopped at its hit, the
// requested AOV layers written.  Included by rg_aov.hip alone (its launcher and the entry points of the
// C ABI), the way rg_render_kernel.h is by the render files: the kernel headers it needs come with it.
#pragma once
#include <hip/hip_runtime.h>

#include "rg_camera.h"
#include "rg_device.h"
#include "rg_k_frames.h"
#include "rg_k_shade.h"
#include "rg_k_trace.h"
#include "rg_launchers.h"

#pragma clang fp contract(off)

using namespace rgk;

#define RG_AOV_BLOCK 256

namespace {

// the 12-byte layers go out as one three-dword store per lane
struct __attribute__((packed, aligned(4))) F3 {
    float x, y, z;
};
struct __attribute__((packed, aligned(4))) F2 {
    float x, y;
};

}  // namespace

// CAMERA: the launch's camera ray, traced by the general closest-hit query (as the camera family of
// rg_render_kernel does); else create_prime's ray through trace_primary and its o = 0 shortcuts.
// F32F / BVH: the query flavour (rg_trace's choice).  SHADE: some layer beyond body and depth is
// requested -- without it the kernel is the trace alone.  Within SHADE a layer that is not requested is
// a wave-uniform branch on its null pointer.
template <bool CAMERA, bool F32F, bool BVH, bool SHADE>
__global__ __launch_bounds__(RG_AOV_BLOCK) void rg_aov_kernel(RgKernelArgs a, RgAovOut o) {
    // the launch context's other counter set starts the next launch at zero (rg_internal.h rg_launch_ctx)
    if (blockIdx.x == 0 && a.counters_next)
        for (uint32_t k = threadIdx.x; k < RG_COUNTER_WORDS; k += RG_AOV_BLOCK) a.counters_next[k] = 0ull;
    __shared__ unsigned int block_prim;
    if (threadIdx.x == 0) block_prim = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t twlog = a.tile_wlog, twmask = (1u << twlog) - 1u, th = 64u >> twlog;
    const uint32_t tiles_x = (a.width + twmask) >> twlog;
    const uint32_t ntiles = tiles_x * ((a.out_rows + th - 1u) / th);
    const uint32_t nwaves = gridDim.x * (RG_AOV_BLOCK / 64u);
    const SphScalar src{rg_cptr(a.sph), rg_cptr(a.sph_cc), rg_cptr(a.sphf), rg_cptr(a.sphf2),
                        rg_cptr(a.pln), rg_cptr(a.dsk), rg_cptr(a.box), rg_cptr(a.nodes), a.lbuf, a.lights};
    uint32_t n_prim = 0;
    for (uint32_t tile = blockIdx.x * (RG_AOV_BLOCK / 64u) + (threadIdx.x >> 6); tile < ntiles; tile += nwaves) {
        const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const uint32_t x = (tx << twlog) + (lane & twmask);
        const uint32_t orow = ty * th + (lane >> twlog);
        const bool inside = x < a.width && orow < a.out_rows;
        const uint32_t y = inside ? out_row_to_y(a, orow) : 0u;
        const size_t oidx = (size_t)orow * a.width + x;
        if (inside && y == 0xFFFFFFFFu) {  // padding row of a partial last tile
            if (o.body) o.body[oidx] = -1;
            if (o.depth) o.depth[oidx] = __builtin_inf();
            if constexpr (SHADE) {
                if (o.normal) reinterpret_cast<F3 *>(o.normal)[oidx] = F3{0.0f, 0.0f, 0.0f};
                if (o.uv) reinterpret_cast<F2 *>(o.uv)[oidx] = F2{0.0f, 0.0f};
                if (o.albedo) reinterpret_cast<F3 *>(o.albedo)[oidx] = F3{0.0f, 0.0f, 0.0f};
            }
        } else if (inside) {
            const uint32_t pixel = y * a.width + x;
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
            if (c.nan && c.nhit >= 2) raise_error(a, pixel, RG_ERR_NAN_DISTANCE);
            const bool hit = c.id >= 0;
            if (o.body) o.body[oidx] = c.id;
            if (o.depth) o.depth[oidx] = hit ? c.t : __builtin_inf();
            if constexpr (SHADE) {
                F3 nrm{0.0f, 0.0f, 0.0f}, alb{a.def[0], a.def[1], a.def[2]};
                F2 uv{0.0f, 0.0f};
                if (hit) {
                    const RgBodyDev b = a.bodies[c.id];
                    const V3 h = add(r.o, scl(r.d, c.t));  // rendering.rs get_color
                    if (o.normal) {
                        V3 n;
                        if (!surface_normal(b, h, n)) raise_error(a, pixel, RG_ERR_AABB_NORMAL);
                        nrm = F3{(float)n.x, (float)n.y, (float)n.z};
                    }
                    if (o.uv || o.albedo) {
                        const RgMatDev m = a.mats[c.id];
                        // only the uv layer and a Texture coloration read the coordinates
                        if (o.uv || m.coloration != RG_COLORATION_COLOR) texture_coords(b, h, uv.x, uv.y);
                        if (o.albedo) {
                            const C3 col = material_color(a.texs, m, uv.x, uv.y);
                            alb = F3{col.r, col.g, col.b};
                        }
                    }
                }
                if (o.normal) reinterpret_cast<F3 *>(o.normal)[oidx] = nrm;
                if (o.uv) reinterpret_cast<F2 *>(o.uv)[oidx] = uv;
                if (o.albedo) reinterpret_cast<F3 *>(o.albedo)[oidx] = alb;
            }
        }
    }
    // ray counter: wave reduction, block reduction in LDS, one atomic per block
    const unsigned long long p64 = wave_sum(n_prim);
    if (lane == 0 && p64) atomicAdd(&block_prim, (unsigned int)p64);
    __syncthreads();
    if (threadIdx.x == 0 && block_prim) atomicAdd(&a.counters[0], (unsigned long long)block_prim);
}
