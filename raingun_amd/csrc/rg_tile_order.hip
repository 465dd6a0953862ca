// rg_tile_order.hip — tile ordering: probe, counting sort and the permutation launcher.
#include <hip/hip_runtime.h>

#include "../../include/raingun.h"
#include "rg_device.h"
#include "rg_k_frames.h"
#include "rg_k_trace.h"
#include "rg_launchers.h"
#include "rg_tile_probe.h"

#pragma clang fp contract(off)

using namespace rgk;

// ---------------------------------------------------------------- tile ordering
// A frame's makespan is max(average work per wave, slowest tile) only if the
// slowest tiles START early; in raster order an expensive band (refractive or
// reflective surfaces: ray trees of up to 2^depth rays per pixel) can start
// late and end the frame alone.  A probe traces 8 primary rays per 8x8 tile
// (NOT counted as rays of the frame), weights each by the material it hits,
// and a counting sort (wave-aggregated histogram, scan, scatter) orders the
// tile queue by descending weight (longest-processing-time-first).  This changes only the
// order in which tiles are dequeued: every pixel is still computed once, by
// the same code, so the output is identical.
// (RG_PROBE_SAMPLES, probe_weight and order_bucket: rg_tile_probe.h, shared with the camera probe)

#define RG_ORDER_CHUNK 1024  // tiles per counting/scatter chunk (one wave each)

// 1) probe: 8 consecutive lanes per tile; writes the tile's bucket
template <bool BVH>
__global__ __launch_bounds__(256) void rg_tile_probe_kernel(RgKernelArgs a, uint32_t *bucket_of, uint32_t ntiles) {
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
        const double sx = a.prim_sx ? a.prim_sx[x]
                                    : ((((double)x + 0.5) / (double)a.width) * 2.0 - 1.0) * a.aspect * a.fov_adjustment;
        const double sy = a.prim_sy ? a.prim_sy[y] : (1.0 - (((double)y + 0.5) / (double)a.height) * 2.0) * a.fov_adjustment;
        trace_primary<true, BVH>(a, src, normalize(v3(sx, sy, -1.0)), c);
        w = probe_weight(a, c);
    }
    w += (uint32_t)__shfl_xor((int)w, 1, 64);
    w += (uint32_t)__shfl_xor((int)w, 2, 64);
    w += (uint32_t)__shfl_xor((int)w, 4, 64);
    if (alive && smp == 0u) bucket_of[tile] = order_bucket(w);
}

// 2) per-chunk bucket histograms (one wave per chunk; no global atomics)
__global__ __launch_bounds__(64) void rg_tile_count_kernel(const uint32_t *bucket_of, uint32_t *chunk_hist,
                                                           uint32_t ntiles) {
    __shared__ uint32_t hist[RG_ORDER_BUCKETS];
    const uint32_t lane = threadIdx.x;
    if (lane < RG_ORDER_BUCKETS) hist[lane] = 0u;
    __syncthreads();
    const uint32_t c0 = blockIdx.x * RG_ORDER_CHUNK, c1 = min(c0 + RG_ORDER_CHUNK, ntiles);
    for (uint32_t t = c0 + lane; t < c1; t += 64u) atomicAdd(&hist[bucket_of[t]], 1u);
    __syncthreads();
    if (lane < RG_ORDER_BUCKETS) chunk_hist[lane * gridDim.x + blockIdx.x] = hist[lane];  // bucket-major: the scan order
}

// 3) exclusive scan in (bucket, chunk) order -> each chunk's first slot per bucket
//    (one block: per-thread serial sums over contiguous ranges, shuffle scans)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
    const int lane = (int)(threadIdx.x & 63u);
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}
__global__ __launch_bounds__(1024) void rg_tile_scan_kernel(uint32_t *chunk_hist, uint32_t nchunks) {
    __shared__ uint32_t wave_tot[16];
    const uint32_t n = nchunks * RG_ORDER_BUCKETS;
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t i0 = threadIdx.x * per, i1 = min(i0 + per, n);
    // chunk_hist is bucket-major (element k = bucket k / nchunks, chunk k % nchunks)
    auto at = [&](uint32_t k) -> uint32_t & { return chunk_hist[k]; };
    uint32_t sum = 0u;
    for (uint32_t k = i0; k < i1; ++k) sum += at(k);
    const uint32_t incl = wave_incl_scan(sum);
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 63u) wave_tot[w] = incl;
    __syncthreads();
    if (w == 0) {
        const uint32_t t = (threadIdx.x < 16u) ? wave_tot[threadIdx.x] : 0u;
        const uint32_t ti = wave_incl_scan(t);
        if (threadIdx.x < 16u) wave_tot[threadIdx.x] = ti - t;  // exclusive wave offsets
    }
    __syncthreads();
    uint32_t run = wave_tot[w] + incl - sum;
    for (uint32_t k = i0; k < i1; ++k) { const uint32_t v = at(k); at(k) = run; run += v; }
}

// 4) stable scatter: one wave walks its chunk in raster order
__global__ __launch_bounds__(64) void rg_tile_scatter_kernel(const uint32_t *bucket_of, const uint32_t *chunk_base,
                                                             uint32_t *perm, uint32_t ntiles) {
    __shared__ uint32_t cur[RG_ORDER_BUCKETS];
    const uint32_t lane = threadIdx.x;
    if (lane < RG_ORDER_BUCKETS) cur[lane] = chunk_base[lane * gridDim.x + blockIdx.x];
    __syncthreads();
    const uint32_t c0 = blockIdx.x * RG_ORDER_CHUNK, c1 = min(c0 + RG_ORDER_CHUNK, ntiles);
    for (uint32_t t0 = c0; t0 < c1; t0 += 64u) {
        const uint32_t t = t0 + lane;
        const bool act = t < c1;
        const uint32_t b = act ? bucket_of[t] : 0u;
        unsigned long long todo = __ballot(act);
        while (todo) {  // one pass per distinct bucket in this group of 64 tiles
            const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
            const uint32_t k = (uint32_t)__shfl((int)b, (int)leader, 64);
            const unsigned long long grp = __ballot(act && b == k);
            if (act && b == k) perm[cur[k] + (uint32_t)__builtin_popcountll(grp & ((1ull << lane) - 1ull))] = t;
            __syncthreads();
            if (lane == leader) cur[k] += (uint32_t)__builtin_popcountll(grp);
            __syncthreads();
            todo &= ~grp;
        }
    }
}

// scratch: [bucket_of ntiles | chunk_hist 64 * nchunks (bucket-major)]
extern "C" size_t rg_tile_order_scratch_words(uint32_t ntiles) {
    const size_t nchunks = (ntiles + RG_ORDER_CHUNK - 1u) / RG_ORDER_CHUNK;
    return (size_t)ntiles + nchunks * RG_ORDER_BUCKETS;
}

extern "C" hipError_t rg_launch_tile_order(const RgKernelArgs *a, uint32_t *scratch, uint32_t *perm, hipStream_t stream) {
    const uint32_t ntiles = (uint32_t)rg_tile_count(*a);
    const uint32_t nchunks = (ntiles + RG_ORDER_CHUNK - 1u) / RG_ORDER_CHUNK;
    uint32_t *bucket_of = scratch, *chunk_hist = scratch + ntiles;
    const uint32_t lanes = ntiles * RG_PROBE_SAMPLES;
    if (a->camera) {  // the camera's rays (rg_tile_order_camera.hip)
        const hipError_t e = rg_launch_tile_probe_camera(a, bucket_of, ntiles, stream);
        if (e != hipSuccess) return e;
    } else if (a->n_nodes > 0)
        hipLaunchKernelGGL(rg_tile_probe_kernel<true>, dim3((lanes + 255u) / 256u), dim3(256), 0, stream, *a, bucket_of,
                           ntiles);
    else
        hipLaunchKernelGGL(rg_tile_probe_kernel<false>, dim3((lanes + 255u) / 256u), dim3(256), 0, stream, *a,
                           bucket_of, ntiles);
    hipLaunchKernelGGL(rg_tile_count_kernel, dim3(nchunks), dim3(64), 0, stream, bucket_of, chunk_hist, ntiles);
    hipLaunchKernelGGL(rg_tile_scan_kernel, dim3(1), dim3(1024), 0, stream, chunk_hist, nchunks);
    hipLaunchKernelGGL(rg_tile_scatter_kernel, dim3(nchunks), dim3(64), 0, stream, bucket_of, chunk_hist, perm, ntiles);
    return hipGetLastError();
}
