// rg_ao_filter.hip — the two image-space kernels of the ambient term (the arithmetic: rg_ambient.h).
// A translation unit of its own, so that every other kernel keeps the device code it had.
//
// 1. rg_ao_filter_kernel<R>: the edge-stopping tent filter of the AO pass, guided by the AOV pass's body and
//    normal layers.  The sum's order is part of the contract (dy outer, dx inner, f32, unfused), so a lane walks
//    the windows of its own pixels in that order and the parallelism is across pixels; the filter is not
//    separable.  A block of 64 x RG_AOF_BY threads makes a tile of 64 x (RG_AOF_BY * RG_AOF_PX) pixels from an
//    LDS copy of the tile plus a halo of R, held as six planes of dwords (ao, body, nx, ny, nz, nn = n . n made
//    once per staged pixel): the 64 lanes of a wave read 64 consecutive dwords of one plane, which no bank sees
//    twice.  A lane makes RG_AOF_PX vertically adjacent pixels of one column: it walks the RG_AOF_PX + 2 R rows
//    its windows cover once, reads each tap's six dwords once and offers the tap to every one of its pixels whose
//    window holds that row -- each pixel still meets its taps in the contract's order.  Entries outside the
//    frame are never read from memory: they are staged with body -1, which no centre with a body accepts (a
//    centre without one keeps its input).  A row's 64 results go out as one 256-B run.
// 2. rg_ambient_compose_kernel: the ambient term added to the beauty frame, one pixel per thread, streaming:
//    28 B read (+ one cached word of the share table) and 4 B (+ 12 B) written per pixel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "rg_ambient.h"
#include "rg_launchers.h"

#pragma clang fp contract(off)

#define RG_AOF_BX 64  // threads across: one wave, one pixel column each
// The open choices, each settled by an A/B build at 4K (profiles/ambient/ab_filter.json; test1 and the
// north star agree to 1 %); the defaults are the winners.  ms at r = 1 / 2 / 4 / 8, waves per block x pixels per lane:
//   8 x 2 (64 x 16 tile)  0.052 / 0.089 / 0.26 / 1.00        4 x 4 (64 x 16)  0.064 / 0.125 / 0.37 / 1.57
//   4 x 2 (64 x 8)        0.055 / 0.093 / 0.29 / 1.19        4 x 1 (64 x 4)   0.061 / 0.116 / 0.30 / 1.16
//   8 x 1 (64 x 8)        0.057 / 0.115 / 0.30 / 1.56       16 x 1 (64 x 16)  0.062 / 0.118 / 0.39 / 1.17
//   2 x 4 (64 x 8)        0.073 / 0.132 / 0.45 / 2.16        2 x 8 (64 x 16)  0.110 / 0.230 / 0.72 / 3.30
// Two pixels per lane beat one (fewer tap reads) and four (the lane's serial chain grows, 68 VGPRs against 44);
// the 16-row tile pays its halo best at r = 8.  At 4 x 4: records 0.064 / 0.123 / 0.36 / 1.58 (a tie with the
// planes; at 8 x 2 0.052 / 0.093 / 0.26 / 0.99), the radius at run time 0.093 / 0.171 / 0.50 / 2.13 (102 VGPRs,
// no unrolled window: a third slower everywhere).
#ifndef RG_AOF_BY
#define RG_AOF_BY 8   // waves per block
#endif
#ifndef RG_AOF_PX
#define RG_AOF_PX 2   // vertically adjacent pixels per lane; the tile is 64 x (RG_AOF_BY * RG_AOF_PX)
#endif
#ifndef RG_AOF_RUNTIME_R
#define RG_AOF_RUNTIME_R 0  // 1: one kernel, the radius a launch argument, dynamic LDS (else eight instantiations)
#endif
#ifndef RG_AOF_RECORD
#define RG_AOF_RECORD 0  // 1: LDS holds {ao, body, nx, ny} as one 16-B and {nz, nn} as one 8-B entry (else six dword planes)
#endif
#define RG_AOF_TH (RG_AOF_BY * RG_AOF_PX)  // tile rows

namespace {

struct RgAoFilterArgs {
    const float *ao;      // H x W
    const int32_t *body;  // H x W
    const float *normal;  // H x W x 3
    float *out;           // H x W
    uint32_t W, H;
    float t;              // normal_min * normal_min
    uint32_t nbx;         // 64-pixel column blocks of a row
    uint32_t r;           // the radius (read by the RG_AOF_RUNTIME_R build only)
};

// One staged pixel.
struct RgAofTap {
    float ao;
    int32_t body;
    float x, y, z, nn;
};

// The tile and its halo in LDS: n entries.
struct RgAofTile {
#if RG_AOF_RECORD
    float4 *a;  // {ao, body, nx, ny}
    float2 *b;  // {nz, nn}
    __device__ __forceinline__ void put(int g, const RgAofTap &t) const {
        a[g] = make_float4(t.ao, __int_as_float(t.body), t.x, t.y);
        b[g] = make_float2(t.z, t.nn);
    }
    __device__ __forceinline__ RgAofTap get(int g) const {
        const float4 u = a[g];
        const float2 v = b[g];
        return RgAofTap{u.x, __float_as_int(u.y), u.z, u.w, v.x, v.y};
    }
#else
    float *ao, *x, *y, *z, *nn;
    int32_t *body;
    __device__ __forceinline__ void put(int g, const RgAofTap &t) const {
        ao[g] = t.ao;
        body[g] = t.body;
        x[g] = t.x;
        y[g] = t.y;
        z[g] = t.z;
        nn[g] = t.nn;
    }
    __device__ __forceinline__ RgAofTap get(int g) const { return RgAofTap{ao[g], body[g], x[g], y[g], z[g], nn[g]}; }
#endif
};

template <int RT>
__global__ __launch_bounds__(RG_AOF_BX *RG_AOF_BY) void rg_ao_filter_kernel(RgAoFilterArgs a) {
    const int R = RG_AOF_RUNTIME_R ? (int)a.r : RT;
    const int TW = RG_AOF_BX + 2 * R, TR = RG_AOF_TH + 2 * R, N = TW * TR;
#if RG_AOF_RUNTIME_R
    extern __shared__ __attribute__((aligned(16))) float lds[];  // 6 N dwords
#else
    constexpr int NMAX = (RG_AOF_BX + 2 * RT) * (RG_AOF_TH + 2 * RT);
    static_assert(NMAX * 24 <= 65536, "the tile and its halo fit a block's LDS");
    __shared__ __attribute__((aligned(16))) float lds[6 * NMAX];
#endif
#if RG_AOF_RECORD
    const RgAofTile tile{reinterpret_cast<float4 *>(lds), reinterpret_cast<float2 *>(lds + 4 * N)};
#else
    const RgAofTile tile{lds, lds + N, lds + 2 * N, lds + 3 * N, lds + 4 * N, reinterpret_cast<int32_t *>(lds + 5 * N)};
#endif
    const int tid = (int)(threadIdx.y * RG_AOF_BX + threadIdx.x);
    const long long W = a.W, H = a.H;
    const long long y0 = (long long)blockIdx.x * RG_AOF_TH;
    for (uint32_t bx = blockIdx.y; bx < a.nbx; bx += gridDim.y) {
        const long long x0 = (long long)bx * RG_AOF_BX;
        for (int g = tid; g < N; g += RG_AOF_BX * RG_AOF_BY) {
            const int r = g / TW, c = g - r * TW;
            const long long y = y0 + r - R, x = x0 + c - R;
            RgAofTap t{0.0f, -1, 0.0f, 0.0f, 0.0f, 0.0f};  // outside the frame: no body, so no centre accepts it
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const size_t q = (size_t)y * a.W + (size_t)x;
                t.ao = a.ao[q];
                t.body = a.body[q];
                t.x = a.normal[3 * q];
                t.y = a.normal[3 * q + 1];
                t.z = a.normal[3 * q + 2];
                t.nn = rg_ambient_dot(t.x, t.y, t.z, t.x, t.y, t.z);
            }
            tile.put(g, t);
        }
        __syncthreads();
        const long long x = x0 + threadIdx.x;
        const int ry0 = (int)threadIdx.y * RG_AOF_PX;  // the lane's first row of the tile
        if (x < W && y0 + ry0 < H) {
            RgAofTap c[RG_AOF_PX];  // the centres
            float sum[RG_AOF_PX];
            int wsum[RG_AOF_PX];
#pragma unroll
            for (int j = 0; j < RG_AOF_PX; ++j) {
                c[j] = tile.get((ry0 + j + R) * TW + (int)threadIdx.x + R);
                sum[j] = 0.0f;
                wsum[j] = 0;
            }
#pragma unroll 1
            for (int rr = 0; rr < RG_AOF_PX + 2 * R; ++rr) {  // staged row ry0 + rr: dy = rr - R - j for pixel j
                const int base = (ry0 + rr) * TW + (int)threadIdx.x;
#pragma unroll
                for (int i = 0; i <= 2 * R; ++i) {  // dx = i - R
                    const RgAofTap q = tile.get(base + i);
#pragma unroll
                    for (int j = 0; j < RG_AOF_PX; ++j) {
                        const int dy = rr - R - j;
                        if (dy < -R || dy > R) continue;
                        const float d = rg_ambient_dot(c[j].x, c[j].y, c[j].z, q.x, q.y, q.z);
                        if ((i == R && dy == 0) || rg_ao_filter_accepts(c[j].body, q.body, d, c[j].nn, q.nn, a.t)) {
                            const int w = rg_ao_filter_weight(R, i - R, dy);
                            sum[j] = sum[j] + (float)w * q.ao;
                            wsum[j] += w;
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < RG_AOF_PX; ++j) {
                const long long y = y0 + ry0 + j;
                if (y < H) a.out[(size_t)y * a.W + (size_t)x] = c[j].body < 0 ? c[j].ao : sum[j] / (float)wsum[j];
            }
        }
        __syncthreads();  // the tile is restaged for the next column block
    }
}

struct RgComposeArgs {
    const float *rgb, *albedo;  // npx x 3
    const int32_t *body;        // npx
    const float *aof;           // npx
    const float *share;         // n_share
    uint32_t *rgba;             // npx
    float *rgb_out;             // nullable (may be rgb): npx x 3
    unsigned long long npx;
    uint32_t n_share;
    float color[3];
};

__global__ __launch_bounds__(256) void rg_ambient_compose_kernel(RgComposeArgs a) {
    const unsigned long long o = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (o >= a.npx) return;
    const int32_t b = a.body[o];
    const bool hit = b >= 0 && (uint32_t)b < a.n_share;
    const float share = hit ? a.share[b] : 0.0f, aof = a.aof[o];
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = rg_ambient_channel(a.rgb[3 * o + c], a.color[c], a.albedo[3 * o + c], share, aof, hit);
    a.rgba[o] = rg_ambient_u8(v[0]) | (rg_ambient_u8(v[1]) << 8) | (rg_ambient_u8(v[2]) << 16) | 0xFF000000u;
    if (a.rgb_out) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.rgb_out[3 * o + c] = v[c];
    }
}

template <int R>
hipError_t launch_r(const RgAoFilterArgs &a, dim3 grid, hipStream_t stream) {
#if RG_AOF_RUNTIME_R
    const size_t lds = (size_t)(RG_AOF_BX + 2 * a.r) * (RG_AOF_TH + 2 * a.r) * 24u;
    hipLaunchKernelGGL((rg_ao_filter_kernel<0>), grid, dim3(RG_AOF_BX, RG_AOF_BY), lds, stream, a);
#else
    hipLaunchKernelGGL((rg_ao_filter_kernel<R>), grid, dim3(RG_AOF_BX, RG_AOF_BY), 0, stream, a);
#endif
    return hipGetLastError();
}

}  // namespace

extern "C" hipError_t rg_launch_ao_filter(const float *ao, const int32_t *body, const float *normal, uint32_t width,
                                          uint32_t height, uint32_t radius, float normal_min, float *out,
                                          hipStream_t stream) {
    if (!ao || !body || !normal || !out || width == 0 || height == 0 || !rg_ao_filter_valid(radius, normal_min))
        return hipErrorInvalidValue;
    RgAoFilterArgs a;
    a.ao = ao;
    a.body = body;
    a.normal = normal;
    a.out = out;
    a.W = width;
    a.H = height;
    a.t = normal_min * normal_min;
    a.r = radius;
    a.nbx = (uint32_t)(((unsigned long long)width + RG_AOF_BX - 1) / RG_AOF_BX);
    const dim3 grid((uint32_t)(((unsigned long long)height + RG_AOF_TH - 1) / RG_AOF_TH), std::min(a.nbx, 65535u));
    switch (radius) {
    case 1: return launch_r<1>(a, grid, stream);
    case 2: return launch_r<2>(a, grid, stream);
    case 3: return launch_r<3>(a, grid, stream);
    case 4: return launch_r<4>(a, grid, stream);
    case 5: return launch_r<5>(a, grid, stream);
    case 6: return launch_r<6>(a, grid, stream);
    case 7: return launch_r<7>(a, grid, stream);
    default: return launch_r<8>(a, grid, stream);
    }
}

extern "C" hipError_t rg_launch_ambient_compose(const float *rgb, const float *albedo, const int32_t *body,
                                                const float *aof, const float *share, uint32_t n_share,
                                                const float color[3], unsigned long long npx, uint8_t *rgba,
                                                float *rgb_out, hipStream_t stream) {
    if (!rgb || !albedo || !body || !aof || !share || !color || !rgba || npx == 0 || npx >= (1ull << 32))
        return hipErrorInvalidValue;
    RgComposeArgs a;
    a.rgb = rgb;
    a.albedo = albedo;
    a.body = body;
    a.aof = aof;
    a.share = share;
    a.rgba = reinterpret_cast<uint32_t *>(rgba);
    a.rgb_out = rgb_out;
    a.npx = npx;
    a.n_share = n_share;
    for (int c = 0; c < 3; ++c) a.color[c] = color[c];
    hipLaunchKernelGGL(rg_ambient_compose_kernel, dim3((unsigned)((npx + 255ull) / 256ull)), dim3(256), 0, stream, a);
    return hipGetLastError();
}
