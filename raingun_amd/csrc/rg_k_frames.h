// rg_k_frames.h — the shading tree's frame stacks, output rows, tile flush and wave sums.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

#include "rg_device.h"
#include "rg_k_math.h"

#pragma clang fp contract(off)

namespace rgk {

// One open node of the shading tree.
struct Frame {
    float f[8];   // REFL: D.rgb, r.  REFR: kr, tau, surf.rgb, Tc.rgb
    double rr[6]; // REFR_T: pending reflection ray (origin, direction)
    int type;
    int cdepth;   // depth of this node's children (task-splitting kernels only: elsewhere a lane's
                  // stack index IS its recursion depth, so frame sp-1's children are at depth sp)
};

// The lane's stack of open frames: at most max_recursion_depth - 1 deep
// (rendering.rs:122-130 stops at depth >= max).  MAXD > 0: a per-lane array
// (scratch).  MAXD == 0 (depths above the largest compiled array,
// scene.rs:16 is a u32): frames live in a global buffer owned by the launch
// context, frame i of the grid's thread g at base[i * stride + g], so frame
// i of a wave is one contiguous run; that launch is persistent, so the grid
// (and the buffer) stays bounded whatever the frame size.
static_assert(sizeof(Frame) == RG_FRAME_BYTES, "host sizes the deep frame buffer with RG_FRAME_BYTES");

template <int MAXD>
struct FrameStack {
    Frame f[MAXD];
    __device__ __forceinline__ void init(const RgKernelArgs &) {}
    __device__ __forceinline__ Frame &operator[](int i) { return f[i]; }
};
// Global frames are stored field-major, like scratch: dword k of frame i of grid
// thread g at plane (i * RG_FRAME_DWORDS + k), element g, so each field access
// of a wave is one coalesced 256-B run (a Frame-struct array would make every
// field a 64-line gather at an 88-B stride).  FrameRefG mirrors Frame's fields.
constexpr int RG_FRAME_DWORDS = (int)(sizeof(Frame) / 4);
static_assert(offsetof(Frame, f) == 0 && offsetof(Frame, rr) == 32 && offsetof(Frame, type) == 80 &&
                  offsetof(Frame, cdepth) == 84 && RG_FRAME_DWORDS == 22,
              "FrameRefG plane numbers");
struct FrameRefG {
    uint32_t *p;      // plane 0 of this frame, this thread
    uint32_t stride;  // dwords between planes (grid threads)
    struct F {        // a float field
        uint32_t *q;
        __device__ __forceinline__ void operator=(float v) const { *q = __float_as_uint(v); }
        __device__ __forceinline__ operator float() const { return __uint_as_float(*q); }
    };
    struct D {        // a double field: two planes
        uint32_t *q;
        uint32_t stride;
        __device__ __forceinline__ void operator=(double v) const {
            const unsigned long long b = (unsigned long long)__double_as_longlong(v);
            q[0] = (uint32_t)b;
            q[stride] = (uint32_t)(b >> 32);
        }
        __device__ __forceinline__ operator double() const {
            return __longlong_as_double((long long)(((unsigned long long)q[stride] << 32) | q[0]));
        }
    };
    struct I {        // an int field
        uint32_t *q;
        __device__ __forceinline__ void operator=(int v) const { *q = (uint32_t)v; }
        __device__ __forceinline__ operator int() const { return (int)*q; }
    };
    struct FA {
        uint32_t *q;
        uint32_t stride;
        __device__ __forceinline__ F operator[](int k) const { return F{q + (size_t)k * stride}; }
    };
    struct DA {
        uint32_t *q;
        uint32_t stride;
        __device__ __forceinline__ D operator[](int k) const { return D{q + (size_t)(2 * k) * stride, stride}; }
    };
    FA f;
    DA rr;
    I type, cdepth;
    __device__ __forceinline__ FrameRefG(uint32_t *p0, uint32_t s)
        : p(p0), stride(s), f{p0, s}, rr{p0 + (size_t)8 * s, s}, type{p0 + (size_t)20 * s},
          cdepth{p0 + (size_t)21 * s} {}
};
template <>
struct FrameStack<0> {
    uint32_t *base;   // plane 0 of frame 0, this thread
    uint32_t stride;  // grid threads
    __device__ __forceinline__ void init(const RgKernelArgs &a) {
        stride = a.deep_stride;
        base = static_cast<uint32_t *>(a.deep_stack) + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    }
    __device__ __forceinline__ FrameRefG operator[](int i) {
        return FrameRefG(base + (size_t)i * RG_FRAME_DWORDS * stride, stride);
    }
};


__device__ __forceinline__ uint32_t out_row_to_y(const RgKernelArgs &a, uint32_t orow) {
    uint32_t tl = orow / a.tile_rows, r = orow - tl * a.tile_rows;
    const unsigned long long i = (unsigned long long)(tl + a.tile_base);
    const unsigned long long ti = a.tile_group > 1u ? (i / a.tile_group) * a.tile_stride + a.tile_offset + i % a.tile_group
                                                    : i * a.tile_stride + a.tile_offset;
    unsigned long long y = ti * a.tile_rows + r;
    return y >= a.height ? 0xFFFFFFFFu : (uint32_t)y;
}

// The same (PLAIN kernels), with the host's shift where tile_rows is a power of two
// (RgKernelArgs::tile_rows_shift; 32: it is not, so its magic, rg_exact.h).
__device__ __forceinline__ uint32_t out_row_to_y_shift(const RgKernelArgs &a, uint32_t orow) {
    const uint32_t tl = a.tile_rows_shift < 32u ? orow >> a.tile_rows_shift : rg_magic_div(orow, a.tile_rows_m, a.tile_rows_sh);
    const uint32_t r = orow - tl * a.tile_rows;
    const unsigned long long i = (unsigned long long)(tl + a.tile_base);
    const unsigned long long ti = a.tile_group > 1u ? (i / a.tile_group) * a.tile_stride + a.tile_offset + i % a.tile_group
                                                    : i * a.tile_stride + a.tile_offset;
    unsigned long long y = ti * a.tile_rows + r;
    return y >= a.height ? 0xFFFFFFFFu : (uint32_t)y;
}

// Output row of the launch's dense row `orow`: itself, or -- one launch of a call split over
// several (RgKernelArgs::out_tile_mul > 1) -- the row of the CALL's selected tile
// (orow / tile_rows) * mul + add that this launch's tile is.
__device__ __forceinline__ uint32_t out_row_of(const RgKernelArgs &a, uint32_t orow) {
    if (a.out_tile_mul <= 1u) return orow;
    const uint32_t tl = orow / a.tile_rows;
    return (tl * a.out_tile_mul + a.out_tile_add) * a.tile_rows + (orow - tl * a.tile_rows);
}

constexpr size_t RG_NO_PIXEL = ~(size_t)0;  // a lane of a tile that lies outside the output

// A wave finished tile `tile`: store its pixels (one coalesced store), then,
// for a consumer on the host (RgKernelArgs::tile_flags), make them visible
// (system-scope release, all lanes) and publish the tile.
__device__ __forceinline__ void flush_tile(const RgKernelArgs &a, size_t oidx, uint32_t px, uint32_t tile, int lane) {
    if (a.defer_px && oidx != RG_NO_PIXEL) a.rgba[oidx] = px;
    if (a.tile_flags) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        if (lane == 0) __hip_atomic_store(&a.tile_flags[tile], a.frame_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__device__ __forceinline__ unsigned long long wave_sum(uint32_t v32) {
    unsigned long long v = v32;
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

}  // namespace rgk
