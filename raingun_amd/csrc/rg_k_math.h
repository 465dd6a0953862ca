// rg_k_math.h — device vector and colour maths, the Rust casts, region counters and error reports
// (the render kernels' headers, rg_k_*.h: see rg_render_kernel.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "rg_device.h"
#include "rg_exact.h"

#pragma clang fp contract(off)

namespace rgk {

constexpr double SHADOW_BIAS = 1e-13;                 // lib.rs:11
constexpr float PI_F = 3.14159265358979323846f;       // std::f32::consts::PI

// MODE_WAIT: the lane's top frame awaits a subtree another lane is tracing (task splitting)
enum : int { MODE_CLOSEST = 0, MODE_SHADOW = 1, MODE_DONE = 2, MODE_WAIT = 3, MODE_SHADOW_H = 4 };
// MODE_SHADOW_H: an idle lane tracing one shadow ray for another lane of its wave (shadow fan-out)
// FR_REFR_TASK / FR_REFR_WAIT carry their pool slot in bits 8+ of Frame::type
enum : int { FR_REFL = 0, FR_REFR_T = 1, FR_REFR_R = 2, FR_REFR_TASK = 4, FR_REFR_WAIT = 5 };

struct V3 { double x, y, z; };
struct C3 { float r, g, b; };

__device__ __forceinline__ V3 v3(double x, double y, double z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 scl(V3 a, double s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ V3 neg(V3 a) { return v3(-a.x, -a.y, -a.z); }
__device__ __forceinline__ double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 normalize(V3 a) { return scl(a, 1.0 / sqrt(dot(a, a))); }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
    return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}

// sqrt(x) and 1.0 / m as hipcc expands them for gfx950 (v_rsq_f64 / v_rcp_f64 and the same fma
// refinement, read off this tree's assembly), WITHOUT the range scaling in front (v_ldexp_f64,
// v_div_scale_f64) and the special-case selects behind (v_cmp_class, v_div_fmas' scale,
// v_div_fixup_f64): for operands the host has bounded (rg_exact.h rg_camera_unscaled_ok) every one
// of those is the identity, so the bits are the expansion's.  10 and 7 instructions for 18 and 12.
__device__ __forceinline__ double sqrt_unscaled(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = y * 0.5;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    g = __builtin_fma(__builtin_fma(-g, g, x), h, g);
    return __builtin_fma(__builtin_fma(-g, g, x), h, g);
}
__device__ __forceinline__ double rcp_unscaled(double m) {
    double r = __builtin_amdgcn_rcp(m);
    r = __builtin_fma(r, __builtin_fma(-m, r, 1.0), r);
    r = __builtin_fma(r, __builtin_fma(-m, r, 1.0), r);
    // the quotient 1.0 * r is r; its residual, times r, on top (v_div_fmas_f64 without its scale)
    return __builtin_fma(__builtin_fma(-m, r, 1.0), r, r);
}

// The same for operands only the lane knows: the lane is admitted by its operand's
// exponent field (rg_exact.h rg_unscaled_ok_hi: biased exponent in [767, 1279], where every scaling
// and fixup of the expansion is the identity), and where any lane of the wave is not, those lanes take
// the compiler's own sqrt / division under a wave-uniform branch -- so a wave of ordinary operands
// never executes the expansion, and 0, denormals, inf, NaN, negative sqrt operands and the far ends
// come out as they always did.  The PLAIN kernels' one use (RG_PLAIN_ULIGHT; 0: as the other kernels,
// for A/B builds): the spherical lights' direction and distance, sqrt_rcp_guarded in rg_k_shade.h
// light_dir_dist.  In sphere_tail, the planes' quotients and fresnel / transmission the same
// primitives measured SLOWER than the compiler's expansions, in the sphere normal no faster, and all
// were taken out again; sqrt_guarded, rcp_guarded and div_guarded stay only as the forms
// rg_debug_unscaled_check proves on the device -- no render kernel calls them.
#ifndef RG_PLAIN_ULIGHT
#define RG_PLAIN_ULIGHT 1
#endif
__device__ __forceinline__ uint32_t high_dword(double x) { return (uint32_t)__double2hiint(x); }
__device__ __forceinline__ double sqrt_guarded(double x) {
    const bool ok = rg_unscaled_ok_hi(high_dword(x));
    double r = sqrt_unscaled(x);
    if (__any(!ok)) {
        if (!ok) r = sqrt(x);
    }
    return r;
}
__device__ __forceinline__ double rcp_guarded(double m) {
    const bool ok = rg_unscaled_ok_abs_hi(high_dword(m));
    double r = rcp_unscaled(m);
    if (__any(!ok)) {
        if (!ok) r = 1.0 / m;
    }
    return r;
}
// m = sqrt(x) and 1.0 / m: an admitted x has m in [2^-128, 2^129), admitted as a divisor
__device__ __forceinline__ void sqrt_rcp_guarded(double x, double &m, double &inv) {
    const bool ok = rg_unscaled_ok_hi(high_dword(x));
    m = sqrt_unscaled(x);
    inv = rcp_unscaled(m);
    if (__any(!ok)) {
        if (!ok) { m = sqrt(x); inv = 1.0 / m; }
    }
}
// a / b: the reciprocal's refinement, q = a r, and one residual step on the quotient -- what hipcc
// emits between v_div_scale_f64 and v_div_fixup_f64, v_div_fmas_f64 without its scale
__device__ __forceinline__ double div_guarded(double a, double b) {
    const bool ok = rg_unscaled_ok_abs_hi(high_dword(a)) && rg_unscaled_ok_abs_hi(high_dword(b));
    double r = __builtin_amdgcn_rcp(b);
    r = __builtin_fma(r, __builtin_fma(-b, r, 1.0), r);
    r = __builtin_fma(r, __builtin_fma(-b, r, 1.0), r);
    double q = a * r;
    q = __builtin_fma(__builtin_fma(-b, q, a), r, q);
    if (__any(!ok)) {
        if (!ok) q = a / b;
    }
    return q;
}
// The primary ray's sensor coordinates (ray.rs:46-51) of pixel (x, y).  _div: the reference's two
// divisions.  _recip (PLAIN kernels): the residual-form quotients of rg_exact.h with the host's
// a.inv_w / a.inv_h, which the launcher admits only after rg_recip_div_ok has compared every
// column's and row's quotient with the division (rg_render_launch.h rg_light_plain).
__device__ __forceinline__ void sensor_div(const RgKernelArgs &a, uint32_t x, uint32_t y, double &sx, double &sy) {
    sx = ((((double)x + 0.5) / a.width_d) * 2.0 - 1.0) * a.aspect * a.fov_adjustment;
    sy = (1.0 - (((double)y + 0.5) / a.height_d) * 2.0) * a.fov_adjustment;
}
__device__ __forceinline__ void sensor_recip(const RgKernelArgs &a, uint32_t x, uint32_t y, double &sx, double &sy) {
    sx = (rg_recip_quot(rg_pixel_centre(x), a.width_d, a.inv_w) * 2.0 - 1.0) * a.aspect * a.fov_adjustment;
    sy = (1.0 - rg_recip_quot(rg_pixel_centre(y), a.height_d, a.inv_h) * 2.0) * a.fov_adjustment;
}
// normalize((sx, sy, -1)) (ray.rs:52-54) with the unscaled expansions: the operand is at least 1
// and bounded by the launcher (rg_camera_unscaled_ok).
__device__ __forceinline__ V3 normalize_camera(double sx, double sy) {
    const V3 d = v3(sx, sy, -1.0);
    return scl(d, rcp_unscaled(sqrt_unscaled(dot(d, d))));
}

__device__ __forceinline__ C3 c3(float r, float g, float b) { return C3{r, g, b}; }
__device__ __forceinline__ C3 cadd(C3 a, C3 b) { return c3(a.r + b.r, a.g + b.g, a.b + b.b); }
__device__ __forceinline__ C3 cmul(C3 a, C3 b) { return c3(a.r * b.r, a.g * b.g, a.b * b.b); }
__device__ __forceinline__ C3 cscl(C3 a, float s) { return c3(a.r * s, a.g * s, a.b * s); }
__device__ __forceinline__ C3 cclamp(C3 a) {  // color.rs:39-43 (f32::min/max ignore NaN)
    return c3(fmaxf(fminf(a.r, 1.0f), 0.0f), fmaxf(fminf(a.g, 1.0f), 0.0f), fmaxf(fminf(a.b, 1.0f), 0.0f));
}

// Rust `f32 as u8` / `f32 as i32`: truncate, saturate, NaN -> 0.
__device__ __forceinline__ uint32_t f32_to_u8(float v) {
    if (!(v > 0.0f)) return 0u;
    if (v >= 255.0f) return 255u;
    return (uint32_t)v;
}
__device__ __forceinline__ int32_t f32_to_i32(float v) {
    if (v != v) return 0;
    if (v >= 2147483648.0f) return 2147483647;
    if (v < -2147483648.0f) return (-2147483647 - 1);
    return (int32_t)v;
}

// Lane l's value of a double (two 32-bit readlanes).
__device__ __forceinline__ double readlane_d(double v, int l) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Region visit counts (diagnostic build -DRG_REGION_STATS; scripts/region_stats.py): every time a
// wave enters region k, its first active lane adds 1 to counters[RG_REGION_BASE + 2k] and the
// active lanes to [+ 2k + 1] -- the dynamic weights of the static ISA budget (scripts/isa_budget.py).
// Words 144.. lie in the lines of tile-queue heads 8-15, unused with RG_NQ = 8.
#define RG_REGION_BASE 144
enum : int {
    RGR_LOOP = 0, RGR_PRIM, RGR_PRIM_SPH_TAIL, RGR_PRIM_PLANE_DIV, RGR_GETCOLOR, RGR_NORMAL_SPHERE,
    RGR_BATCH, RGR_TEXEL, RGR_UV_SPHERE, RGR_UV_PLANE, RGR_LIGHT_SPH, RGR_REFRACT, RGR_SHADE, RGR_UNWIND,
    RGR_UNWIND_STEP, RGR_TILE_FETCH, RGR_Q_CLOSEST, RGR_Q_SHADOW, RGR_SH_GROUP, RGR_SH_TAIL, RGR_SH_PLANE,
    RGR_SH_PLANE_DIV, RGR_QC_GROUP, RGR_QC_TAIL, RGR_QC_PLANE, RGR_PRIM_GROUP, RGR_PRIM_PLANE, RGR_DISK, RGR_BOX,
    RGR_PUSH_REFL, RGR_PUSH_REFR, RGR_UNWIND_REFRT, RGR_ERROR, RGR_SH_PAIR, RGR_PRIM_PAIR, RGR_QC_PAIR,
    RGR_WALK, RGR_WALK_LEAF, RGR_LB_SHADOW, RGR_FIRST_HIT, RGR_COUNT
};
static_assert(RG_REGION_BASE + 2 * RGR_COUNT <= 16 + 16 * 15, "region counters stay below tile-queue head 15");
#ifdef RG_REGION_STATS
#define RG_REGION(k)                                                                                  \
    do {                                                                                              \
        const unsigned long long m_ = __ballot(1);                                                    \
        if ((int)(threadIdx.x & 63u) == __builtin_ffsll((long long)m_) - 1) {                         \
            atomicAdd(&a.counters[RG_REGION_BASE + 2 * (k)], 1ull);                                   \
            atomicAdd(&a.counters[RG_REGION_BASE + 2 * (k) + 1], (unsigned long long)__builtin_popcountll(m_)); \
        }                                                                                             \
    } while (0)
#else
#define RG_REGION(k) do { } while (0)
#endif

__device__ __forceinline__ void raise_error(const RgKernelArgs &a, uint32_t pixel, int status) {
    RG_REGION(RGR_ERROR);
    // lowest pixel wins: max of the complemented key; 0 (memset) = no error
    unsigned long long key = ((unsigned long long)pixel << 8) | (unsigned long long)(-status);
    atomicMax(&a.counters[3], ~key);
    if (a.err_sticky) atomicMax(a.err_sticky, ~key);  // survives the next launch's counter reset
}

}  // namespace rgk
