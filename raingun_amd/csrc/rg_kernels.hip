// rg_kernels.hip — the render launchers: the occupancy cache, the choice of a compiled
// rg_render_kernel group (frame-stack depth, path: rg_render_launch.h, rg_render_*.hip) and
// the extern "C" entry points; rg_trace_kernel (Scene::trace for a batch of rays).
// The megakernel itself: rg_render_kernel.h.  Tile ordering: rg_tile_order.hip.
#include <hip/hip_runtime.h>

#include <mutex>
#include <utility>
#include <vector>

#include "rg_device.h"
#include "rg_k_trace.h"
#include "rg_launchers.h"
#include "rg_render_launch.h"

#pragma clang fp contract(off)

using namespace rgk;

// Scene::trace for a batch of rays (rg_trace): one lane per ray.
__global__ __launch_bounds__(256) void rg_trace_kernel(RgKernelArgs a, const double *rays, uint32_t n,
                                                       double *dist, int32_t *body) {
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool alive = i < n;
    Ray r;
    r.o = v3(0, 0, 0);
    r.d = v3(0, 0, 1);
    if (alive) {
        r.o = v3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]);
        r.d = v3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    }
    Closest c;
    closest_init(c);
    bool occl = false;
    if (alive) {
        SphScalar src{rg_cptr(a.sph), rg_cptr(a.sph_cc), rg_cptr(a.sphf), rg_cptr(a.sphf2),
                      rg_cptr(a.pln), rg_cptr(a.dsk), rg_cptr(a.box), rg_cptr(a.nodes), a.lbuf, a.lights};
        if (a.n_nodes > 0) trace_query<true, true>(a, src, r, false, 0.0, c, occl, a.lane_min_depth <= 1);
        else if (a.path == RG_PATH_HEAVY) trace_query<true, false>(a, src, r, false, 0.0, c, occl);
        else trace_query<false, false>(a, src, r, false, 0.0, c, occl);
        if (c.nan && c.nhit >= 2) raise_error(a, i, RG_ERR_NAN_DISTANCE);
        dist[i] = c.id >= 0 ? c.t : 0.0;
        body[i] = c.id;
    }
}

// rg_debug_camera_check: every pixel's camera direction as the general kernels compute it (two
// divisions, normalize) and as the PLAIN kernels do (rg_k_math.h sensor_recip, normalize_camera);
// *bad counts the pixels whose directions differ in any bit.  One lane per pixel; reads a.width,
// a.height, the frame constants and a.inv_w / a.inv_h only.
__global__ __launch_bounds__(256) void rg_camera_check_kernel(RgKernelArgs a, unsigned long long *bad) {
    const unsigned long long p = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (p >= (unsigned long long)a.width * a.height) return;
    const uint32_t y = (uint32_t)(p / a.width), x = (uint32_t)(p - (unsigned long long)y * a.width);
    double sx, sy;
    sensor_div(a, x, y, sx, sy);
    const V3 d0 = normalize(v3(sx, sy, -1.0));
    sensor_recip(a, x, y, sx, sy);
    const V3 d1 = normalize_camera(sx, sy);
    if (__double_as_longlong(d0.x) != __double_as_longlong(d1.x) || __double_as_longlong(d0.y) != __double_as_longlong(d1.y) ||
        __double_as_longlong(d0.z) != __double_as_longlong(d1.z))
        atomicAdd(bad, 1ull);
}

extern "C" hipError_t rg_launch_camera_check(const RgKernelArgs *a, unsigned long long *bad, hipStream_t stream) {
    const unsigned long long n = (unsigned long long)a->width * a->height;
    if (n == 0 || n >= (1ull << 32)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rg_camera_check_kernel, dim3((unsigned)((n + 255ull) / 256ull)), dim3(256), 0, stream, *a, bad);
    return hipGetLastError();
}

// rg_debug_unscaled_check: the guarded primitives of rg_k_math.h (the PLAIN kernels' sqrt, 1.0 / x and
// a / b: unscaled for the lanes whose operands admit it, the compiler's own under a wave-uniform branch
// for the rest) against the compiler's sqrt and division, one lane per operand.  Two kernels, so that
// neither side's code can be merged with the other's: the first stores the guarded results, the
// second computes the plain ones and counts the operands whose results differ in any bit.
// op: 0 sqrt(a), 1 1.0 / a, 2 a / b, 3 sqrt(a) and 1.0 / sqrt(a) from one admission (out[i], out[n + i]).
__global__ __launch_bounds__(256) void rg_unscaled_guarded_kernel(int op, const double *a, const double *b, uint32_t n,
                                                                  double *out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const double x = a[i];
    if (op == 0) out[i] = sqrt_guarded(x);
    else if (op == 1) out[i] = rcp_guarded(x);
    else if (op == 2) out[i] = div_guarded(x, b[i]);
    else sqrt_rcp_guarded(x, out[i], out[n + i]);
}
__global__ __launch_bounds__(256) void rg_unscaled_compare_kernel(int op, const double *a, const double *b, uint32_t n,
                                                                  const double *out, unsigned long long *bad) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const double x = a[i];
    bool same;
    if (op == 0) same = __double_as_longlong(sqrt(x)) == __double_as_longlong(out[i]);
    else if (op == 1) same = __double_as_longlong(1.0 / x) == __double_as_longlong(out[i]);
    else if (op == 2) same = __double_as_longlong(x / b[i]) == __double_as_longlong(out[i]);
    else {
        const double m = sqrt(x);
        same = __double_as_longlong(m) == __double_as_longlong(out[i]) &&
               __double_as_longlong(1.0 / m) == __double_as_longlong(out[n + i]);
    }
    if (!same) atomicAdd(bad, 1ull);
}

extern "C" hipError_t rg_launch_unscaled_check(int op, const double *a, const double *b, uint32_t n, double *out,
                                               unsigned long long *bad, hipStream_t stream) {
    if (n == 0 || op < 0 || op > 3) return hipErrorInvalidValue;
    const dim3 grid((n + 255u) / 256u);
    hipLaunchKernelGGL(rg_unscaled_guarded_kernel, grid, dim3(256), 0, stream, op, a, b, n, out);
    hipLaunchKernelGGL(rg_unscaled_compare_kernel, grid, dim3(256), 0, stream, op, a, b, n, out, bad);
    return hipGetLastError();
}

// ---------------------------------------------------------------- launchers
// Occupancy of one kernel instantiation on the CURRENT device, cached per
// (device, kernel, dynamic LDS): hipFuncSetAttribute and the occupancy query
// are per device, and scenes on different devices (rg_render_multi) or host
// threads may launch the same instantiation.
struct OccKey {
    int dev;
    const void *kern;
    size_t lds;
};
static std::mutex occ_mu;
static std::vector<std::pair<OccKey, std::pair<int, int>>> occ_cache;  // -> (CUs, blocks per CU)

hipError_t occupancy(const void *kern, int threads, size_t lds, int &cus, int &per_cu) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> g(occ_mu);
    for (const auto &e : occ_cache)
        if (e.first.dev == dev && e.first.kern == kern && e.first.lds == lds) {
            cus = e.second.first;
            per_cu = e.second.second;
            return hipSuccess;
        }
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return hipErrorInvalidValue;
    if (lds > 64 * 1024 && hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return hipErrorInvalidValue;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds) != hipSuccess)
        return hipErrorInvalidValue;
    if (per_cu < 1) return hipErrorInvalidConfiguration;
    occ_cache.push_back({OccKey{dev, kern, lds}, {cus, per_cu}});
    return hipSuccess;
}

// Frame-stack capacity of each compiled array instantiation; deeper scenes use
// the global frame buffer (MAXD == 0).
extern "C" int rg_max_array_frames(void) { return 64; }

// Host-frame launches (pixels into page-locked host memory, tile publication,
// cancellation, other tile shapes) of heavy-path scenes needing at most this
// many frames run array-frame kernels with the host-frame features (HF:
// north star into pinned memory 2.59 -> 2.53 ms, profiles/r05/s15); deeper
// ones and light-path scenes the MAXD == 0 kernels (light HF measured slower:
// test1 0.878 -> 0.895 ms, 9 spills).
#ifndef RG_HOST_ARRAY_FRAMES
#define RG_HOST_ARRAY_FRAMES 8
#endif
extern "C" int rg_host_array_frames(void) { return RG_HOST_ARRAY_FRAMES; }

static bool host_frame_launch(const RgKernelArgs *a) {
    return a->defer_px || a->tile_flags || a->cancel || a->image_rows || a->tile_wlog != 3u;
}

// Does this launch keep its frames in the launch context's global buffer (the
// host sizes it with rg_render_grid_threads)?  Depths above the arrays, sparse and camera launches.
extern "C" int rg_launch_global_frames(const RgKernelArgs *a, int maxd) {
    return a->px_mask != nullptr || a->camera != 0 || maxd > rg_max_array_frames();
}

template <int MAXD, bool HF = false>
static hipError_t launch_depth(const RgKernelArgs *a, hipStream_t stream, size_t *gt, int *plain) {
    if (rg_heavy_path(*a)) return launch_heavy<MAXD, HF>(a, stream, gt);
    // light host frames run the MAXD == 0 kernels: array-frame HF light kernels (9 spilled
    // VGPRs) measured slower into pinned memory, 0.768 -> 0.826 ms (profiles/r06/s5)
    if constexpr (HF) return hipErrorInvalidValue;
    else return launch_light<MAXD>(a, stream, gt, plain);
}

// plain (nullable): whether the launch runs a PLAIN light instantiation (rg_render_launch.h rg_light_plain)
static hipError_t dispatch_depth(const RgKernelArgs *a, int maxd, hipStream_t stream, size_t *gt, int *plain = nullptr) {
    if (plain) *plain = 0;
    if (a->area_tab)  // a band of a supersampled frame with area lights (rg_render_*_area.hip): the lens family's launch, lights per sample
        return rg_heavy_path(*a) ? launch_heavy<RG_MAXD_AREA, false>(a, stream, gt) : launch_light<RG_MAXD_AREA>(a, stream, gt, plain);
    if (a->lens)  // a band of a supersampled frame through a thin lens (rg_render_*_lens.hip): the camera family's launch, lens rays
        return rg_heavy_path(*a) ? launch_heavy<RG_MAXD_LENS, false>(a, stream, gt) : launch_light<RG_MAXD_LENS>(a, stream, gt, plain);
    if (a->camera) {  // a camera launch (rg_render_*_camera*.hip): primary rays from the eye, frames in the global buffer
        if (a->px_mask)
            return rg_heavy_path(*a) ? launch_heavy<RG_MAXD_CAMERA, false, true>(a, stream, gt)
                                     : launch_light<RG_MAXD_CAMERA, true>(a, stream, gt, plain);
        return rg_heavy_path(*a) ? launch_heavy<RG_MAXD_CAMERA, false>(a, stream, gt)
                                 : launch_light<RG_MAXD_CAMERA>(a, stream, gt, plain);
    }
    if (a->px_mask)  // a sparse launch (rg_render_*_sparse.hip): a tile list and a pixel mask, frames in the global buffer
        return rg_heavy_path(*a) ? launch_heavy<0, false, true>(a, stream, gt) : launch_light<0, true>(a, stream, gt, plain);
    if (host_frame_launch(a)) {
        if (RG_HOST_ARRAY_FRAMES > 0 && maxd <= RG_HOST_ARRAY_FRAMES && rg_heavy_path(*a))
            return launch_depth<8, true>(a, stream, gt, plain);
        return launch_depth<0>(a, stream, gt, plain);
    }
    if (maxd <= 8) return launch_depth<8>(a, stream, gt, plain);
    if (maxd <= 16) return launch_depth<16>(a, stream, gt, plain);
    if (maxd <= 64) return launch_depth<64>(a, stream, gt, plain);
    return launch_depth<0>(a, stream, gt, plain);
}

extern "C" hipError_t rg_launch_render(const RgKernelArgs *a, int maxd, hipStream_t stream, int *plain) {
    return dispatch_depth(a, maxd, stream, nullptr, plain);
}

// Threads of the grid rg_launch_render would use (frame-buffer sizing for maxd > 64).
extern "C" hipError_t rg_render_grid_threads(const RgKernelArgs *a, int maxd, size_t *threads) {
    return dispatch_depth(a, maxd, nullptr, threads);
}

extern "C" hipError_t rg_launch_trace(const RgKernelArgs *a, const double *rays, uint32_t n, double *dist,
                                      int32_t *body, hipStream_t stream) {
    dim3 grid((n + 255) / 256);
    // per-lane walk stacks (stride = block size): lane_stack entries + the spare slot
    const size_t lds = a->lane_stack > 0 ? ((size_t)(a->lane_stack + 1) * 4u) * 256u : 0u;
    hipLaunchKernelGGL(rg_trace_kernel, grid, dim3(256), lds, stream, *a, rays, n, dist, body);
    return hipGetLastError();
}
