// rg_resolve.hip — the box resolve of supersampled frames (rg_render_image_aa /
// rg_render_aa_async / rg_resolve_box, rg_aa.hip): k x k packed f32 RGB samples per
// output pixel in, RGBA8 and (optionally) the f32 mean out.  The arithmetic is
// fixed (raingun_amd/aa.py restates it in numpy and the tests compare bit for bit):
//   clamp   s' = s if 0 <= s <= 1, 1 if s > 1, else 0 (negatives and NaN: `f32 as u8`, color.rs:32-37)
//   sum     acc = 0; acc = acc + s'[j][i], sample rows j outer, columns i inner, f32, unfused
//   mean    acc / (float)(k k), an IEEE division
//   byte    f32_to_u8(mean * 255), alpha 255
// A pure streaming kernel: every sample is read once, nothing is reused.  A thread
// makes RG_RESOLVE_PX adjacent output pixels of one row, so it reads 4 k samples =
// 48 k contiguous bytes per sample row (3 k 16-B loads when the sample row pitch
// k W 12 B is a multiple of 16, dword loads otherwise) and a wave reads one
// contiguous run of 3 k KiB per sample row; it writes its four RGBA8 pixels as one
// 16-B store and the f32 means as three (when W is a multiple of 4, else dwords).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "rg_launchers.h"

#pragma clang fp contract(off)

#define RG_RESOLVE_PX 4   // adjacent output pixels per thread
#define RG_RESOLVE_BX 64  // threads across (one wave: 256 output pixels)
#define RG_RESOLVE_BY 4   // output rows per block

namespace {

struct RgResolveArgs {
    const float *in;    // k rows x (k W) samples x 3 floats, packed
    uint32_t *rgba;     // rows x W
    float *rgb;         // nullable: rows x W x 3
    uint32_t W, rows;   // output pixels per row, output rows
    uint32_t vec_out;   // W % 4 == 0 and both outputs 16-B aligned: 16-B stores
};

// Rust `f32 as u8`: truncate, saturate, NaN -> 0 (rg_k_math.h f32_to_u8).
__device__ __forceinline__ uint32_t resolve_u8(float v) {
    if (!(v > 0.0f)) return 0u;
    if (v >= 255.0f) return 255u;
    return (uint32_t)v;
}

__device__ __forceinline__ float resolve_clamp(float s) {
    return (s >= 0.0f && s <= 1.0f) ? s : (s > 1.0f ? 1.0f : 0.0f);
}

// One output pixel on its own (the last, partial group of a row): dword loads and stores.
template <int K>
__device__ __forceinline__ void resolve_one(const RgResolveArgs &a, const float *row, size_t pitch, size_t o) {
    float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int j = 0; j < K; ++j, row += pitch)
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = acc[c] + resolve_clamp(row[i * 3 + c]);
    float mean[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) mean[c] = acc[c] / (float)(K * K);
    a.rgba[o] = resolve_u8(mean[0] * 255.0f) | (resolve_u8(mean[1] * 255.0f) << 8) |
                (resolve_u8(mean[2] * 255.0f) << 16) | 0xFF000000u;
    if (a.rgb) {
        a.rgb[3 * o] = mean[0];
        a.rgb[3 * o + 1] = mean[1];
        a.rgb[3 * o + 2] = mean[2];
    }
}

// K: samples per pixel side; VIN: sample rows are 16-B aligned at every thread's first sample.
template <int K, bool VIN>
__global__ __launch_bounds__(RG_RESOLVE_BX *RG_RESOLVE_BY) void rg_resolve_kernel(RgResolveArgs a) {
    constexpr int P = RG_RESOLVE_PX, NF = P * K * 3;  // floats a thread reads per sample row
    constexpr int UJ = K <= 2 ? K : 1;                // unroll factor of the loop over sample rows
    const uint32_t x0 = (blockIdx.x * RG_RESOLVE_BX + threadIdx.x) * P;
    const uint32_t y = blockIdx.y * RG_RESOLVE_BY + threadIdx.y;
    if (x0 >= a.W || y >= a.rows) return;
    const size_t pitch = (size_t)a.W * (K * 3);  // floats per sample row
    const float *row = a.in + (size_t)y * K * pitch + (size_t)x0 * (K * 3);
    const size_t o = (size_t)y * a.W + x0;
    if (a.W - x0 < (uint32_t)P) {  // the row's last thread when W is no multiple of 4: 1..3 pixels
        for (uint32_t p = 0; p < a.W - x0; ++p) resolve_one<K>(a, row + (size_t)p * (K * 3), pitch, o + p);
        return;
    }
    float acc[P * 3];
#pragma unroll
    for (int q = 0; q < P * 3; ++q) acc[q] = 0.0f;
    // one sample row's loads in flight per thread from k = 3 on: unrolled over the rows, the
    // compiler hoists all k x 12 k loads and the kernel runs at 1-2 waves per SIMD (k >= 7 spills)
#pragma unroll UJ
    for (int j = 0; j < K; ++j, row += pitch) {
        float v[NF];
        if (VIN) {
            const float4 *r4 = reinterpret_cast<const float4 *>(row);
#pragma unroll
            for (int m = 0; m < NF / 4; ++m) {
                const float4 t = r4[m];
                v[4 * m] = t.x; v[4 * m + 1] = t.y; v[4 * m + 2] = t.z; v[4 * m + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int f = 0; f < NF; ++f) v[f] = row[f];
        }
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int i = 0; i < K; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[p * 3 + c] = acc[p * 3 + c] + resolve_clamp(v[(p * K + i) * 3 + c]);
    }
    float mean[P * 3];
    uint32_t px[P];
#pragma unroll
    for (int q = 0; q < P * 3; ++q) mean[q] = acc[q] / (float)(K * K);
#pragma unroll
    for (int p = 0; p < P; ++p)
        px[p] = resolve_u8(mean[3 * p] * 255.0f) | (resolve_u8(mean[3 * p + 1] * 255.0f) << 8) |
                (resolve_u8(mean[3 * p + 2] * 255.0f) << 16) | 0xFF000000u;
    if (a.vec_out) {
        *reinterpret_cast<uint4 *>(a.rgba + o) = make_uint4(px[0], px[1], px[2], px[3]);
        if (a.rgb) {
            float4 *d = reinterpret_cast<float4 *>(a.rgb + 3 * o);
#pragma unroll
            for (int m = 0; m < 3; ++m) d[m] = make_float4(mean[4 * m], mean[4 * m + 1], mean[4 * m + 2], mean[4 * m + 3]);
        }
    } else {
#pragma unroll
        for (int p = 0; p < P; ++p) a.rgba[o + p] = px[p];
        if (a.rgb) {
#pragma unroll
            for (int q = 0; q < P * 3; ++q) a.rgb[3 * o + q] = mean[q];
        }
    }
}

// The resolve of adaptive anti-aliasing (rg_aa.hip): per output pixel of a band, one thread.
// A flagged pixel (mask byte non-zero, `in` non-null) is the box resolve of its k x k samples
// in resolve_one's order and arithmetic, from the band's sample slot (only the samples of
// flagged pixels were rendered there); an unflagged pixel keeps the base frame's bytes, and
// its base f32 RGB is clamped in place when `rgb` is wanted (the k = 1 resolve).  Per wave:
// 64 mask bytes read; per flagged lane k runs of 12 k B read (adjacent flagged lanes read one
// contiguous run per sample row), 4 B (+ 12 B) written; with `rgb`, 12 B read and written per
// unflagged lane.  Flagged pixels are a small share of the frame, so the shape is the simple one.
struct RgAdaptArgs {
    const float *in;      // nullable (k = 1: nothing to resolve): k rows x (k W) samples x 3 floats
    const uint8_t *mask;  // rows x W
    uint32_t *rgba;       // rows x W, holding the base frame
    float *rgb;           // nullable: rows x W x 3, holding the base frame's f32 RGB
    uint32_t W, rows, k;
};

__global__ __launch_bounds__(256) void rg_resolve_adaptive_kernel(RgAdaptArgs a) {
    const size_t o = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (o >= (size_t)a.W * a.rows) return;
    if (a.in && a.mask[o]) {
        const uint32_t y = (uint32_t)(o / a.W), x = (uint32_t)(o - (size_t)y * a.W);
        const size_t pitch = (size_t)a.W * a.k * 3;  // floats per sample row
        const float *row = a.in + (size_t)y * a.k * pitch + (size_t)x * a.k * 3;
        float acc[3] = {0.0f, 0.0f, 0.0f};
        for (uint32_t j = 0; j < a.k; ++j, row += pitch)
            for (uint32_t i = 0; i < a.k; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = acc[c] + resolve_clamp(row[i * 3 + c]);
        float mean[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) mean[c] = acc[c] / (float)(a.k * a.k);
        a.rgba[o] = resolve_u8(mean[0] * 255.0f) | (resolve_u8(mean[1] * 255.0f) << 8) |
                    (resolve_u8(mean[2] * 255.0f) << 16) | 0xFF000000u;
        if (a.rgb) {
            a.rgb[3 * o] = mean[0];
            a.rgb[3 * o + 1] = mean[1];
            a.rgb[3 * o + 2] = mean[2];
        }
    } else if (a.rgb) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.rgb[3 * o + c] = resolve_clamp(a.rgb[3 * o + c]);
    }
}

template <int K>
hipError_t launch_k(const RgResolveArgs &a, bool vin, dim3 grid, hipStream_t stream) {
    const dim3 block(RG_RESOLVE_BX, RG_RESOLVE_BY);
    if (vin) hipLaunchKernelGGL((rg_resolve_kernel<K, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((rg_resolve_kernel<K, false>), grid, block, 0, stream, a);
    return hipGetLastError();
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" hipError_t rg_launch_resolve(const float *in, uint32_t width, uint32_t rows, uint32_t k, uint8_t *rgba,
                                        float *rgb, hipStream_t stream) {
    if (!in || !rgba || width == 0 || k < 1 || k > 8) return hipErrorInvalidValue;
    const bool vin = ((unsigned long long)k * width) % 4 == 0 && aligned16(in);
    const uint32_t vec_out = (width % 4 == 0 && aligned16(rgba) && (!rgb || aligned16(rgb))) ? 1u : 0u;
    const uint32_t gx = (width + RG_RESOLVE_PX * RG_RESOLVE_BX - 1) / (RG_RESOLVE_PX * RG_RESOLVE_BX);
    const size_t pitch = (size_t)k * width * 3;
    // grids of at most 65535 blocks down: slices of whole blocks' rows (16-B alignment holds per
    // row when it holds for the first)
    const uint32_t slice = 65535u * RG_RESOLVE_BY;
    for (uint32_t r0 = 0; r0 < rows; r0 += slice) {
        RgResolveArgs a;
        a.in = in + (size_t)r0 * k * pitch;
        a.rgba = reinterpret_cast<uint32_t *>(rgba) + (size_t)r0 * width;
        a.rgb = rgb ? rgb + (size_t)r0 * width * 3 : nullptr;
        a.W = width;
        a.rows = std::min(slice, rows - r0);
        a.vec_out = vec_out;
        const dim3 grid(gx, (a.rows + RG_RESOLVE_BY - 1) / RG_RESOLVE_BY);
        hipError_t e = hipSuccess;
        switch (k) {
        case 1: e = launch_k<1>(a, vin, grid, stream); break;
        case 2: e = launch_k<2>(a, vin, grid, stream); break;
        case 3: e = launch_k<3>(a, vin, grid, stream); break;
        case 4: e = launch_k<4>(a, vin, grid, stream); break;
        case 5: e = launch_k<5>(a, vin, grid, stream); break;
        case 6: e = launch_k<6>(a, vin, grid, stream); break;
        case 7: e = launch_k<7>(a, vin, grid, stream); break;
        default: e = launch_k<8>(a, vin, grid, stream); break;
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

extern "C" hipError_t rg_launch_resolve_adaptive(const float *in, const uint8_t *mask, uint32_t width, uint32_t rows,
                                                 uint32_t k, uint8_t *rgba, float *rgb, hipStream_t stream) {
    if (!mask || !rgba || width == 0 || k < 1 || k > 8) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    const RgAdaptArgs a{in, mask, reinterpret_cast<uint32_t *>(rgba), rgb, width, rows, k};
    const size_t px = (size_t)width * rows;  // < 2^32: the grid stays below 2^24 blocks
    hipLaunchKernelGGL(rg_resolve_adaptive_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}
