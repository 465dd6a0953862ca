// rg_tile_order_camera.hip — the tile-order probe of a camera launch (rg_scene_set_camera; rg_camera.h):
// the samples of rg_tile_order.hip's probe, each the camera's ray through its pixel, traced by the
// general closest-hit query (nothing of trace_primary's o = 0 holds for it).  In a translation unit
// of its own, as the camera's render kernels are: rg_tile_order.hip keeps the device code it had.
#include <hip/hip_runtime.h>

#include "rg_camera.h"
#include "rg_launchers.h"
#include "rg_tile_probe.h"

#pragma clang fp contract(off)

// 8 consecutive lanes per tile; writes the tile's bucket (rg_tile_order.hip rg_tile_probe_kernel)
template <bool BVH>
__global__ __launch_bounds__(256) void rg_tile_probe_camera_kernel(RgKernelArgs a, uint32_t *bucket_of, uint32_t ntiles) {
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    const uint32_t tile = gid / RG_PROBE_SAMPLES, smp = gid % RG_PROBE_SAMPLES;
    const uint32_t tiles_x = rg_tiles_x(a), tw = rg_tile_w(a), th = rg_tile_h(a);
    bool alive = tile < ntiles;
    const uint32_t ty = alive ? tile / tiles_x : 0u, tx = alive ? tile - ty * tiles_x : 0u;
    // corners and inner points of an 8x8 tile, scaled to the tile's shape
    const uint32_t ox8 = (smp & 3u) == 0u ? 0u : (smp & 3u) == 1u ? 7u : (smp & 3u) == 2u ? 2u : 5u;
    const uint32_t oy8 = smp < 4u ? ((smp & 1u) ? 7u : 0u) : ((smp & 1u) ? 5u : 2u);
    const uint32_t x = min(tx * tw + ox8 * (tw - 1u) / 7u, a.width - 1u);
    const uint32_t orow = min(ty * th + oy8 * (th - 1u) / 7u, a.out_rows - 1u);
    const uint32_t y = alive ? out_row_to_y(a, orow) : 0u;
    uint32_t w = 0u;
    if (alive && y != 0xFFFFFFFFu) {
        Closest c;
        closest_init(c);
        SphScalar src{rg_cptr(a.sph), rg_cptr(a.sph_cc), rg_cptr(a.sphf), rg_cptr(a.sphf2),
                      rg_cptr(a.pln), rg_cptr(a.dsk), rg_cptr(a.box), rg_cptr(a.nodes), a.lbuf, a.lights};
        double sx, sy, dir[3];
        rg_camera_sensor(x, y, a.width_d, a.height_d, a.aspect, a.fov_adjustment, &sx, &sy);
        rg_camera_direction(a.cam_right, a.cam_up, a.cam_forward, sx, sy, dir);
        Ray r;
        r.o = v3(a.cam_eye[0], a.cam_eye[1], a.cam_eye[2]);
        r.d = v3(dir[0], dir[1], dir[2]);
        bool occl = false;
        trace_query<true, BVH>(a, src, r, false, 0.0, c, occl);
        w = probe_weight(a, c);
    }
    w += (uint32_t)__shfl_xor((int)w, 1, 64);
    w += (uint32_t)__shfl_xor((int)w, 2, 64);
    w += (uint32_t)__shfl_xor((int)w, 4, 64);
    if (alive && smp == 0u) bucket_of[tile] = order_bucket(w);
}

extern "C" hipError_t rg_launch_tile_probe_camera(const RgKernelArgs *a, uint32_t *bucket_of, uint32_t ntiles,
                                                  hipStream_t stream) {
    const uint32_t lanes = ntiles * RG_PROBE_SAMPLES;
    if (a->n_nodes > 0)
        hipLaunchKernelGGL(rg_tile_probe_camera_kernel<true>, dim3((lanes + 255u) / 256u), dim3(256), 0, stream, *a,
                           bucket_of, ntiles);
    else
        hipLaunchKernelGGL(rg_tile_probe_camera_kernel<false>, dim3((lanes + 255u) / 256u), dim3(256), 0, stream, *a,
                           bucket_of, ntiles);
    return hipGetLastError();
}
