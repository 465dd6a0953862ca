// rg_k_shade.h — normals, texture coordinates and lookup, Fresnel, reflection, transmission, lights.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/raingun.h"
#include "rg_device.h"
#include "rg_k_intersect.h"
#include "rg_k_math.h"

#pragma clang fp contract(off)

namespace rgk {

// ---------------------------------------------------------------- shading
__device__ __forceinline__ V3 bp3(const RgBodyDev &b, int k) { return v3(b.p[k], b.p[k + 1], b.p[k + 2]); }

// bodies.rs:122-124, 151-153, 194-196, 284-328.  false = the AABB assert.
__device__ __forceinline__ bool surface_normal(const RgBodyDev &b, V3 h, V3 &n) {
    if (b.kind == RG_BODY_SPHERE) { n = normalize(sub(h, bp3(b, 0))); return true; }
    if (b.kind != RG_BODY_AABB) { n = neg(bp3(b, 3)); return true; }
    if (fabs(h.x - b.p[0]) < 1e-8) n = v3(-1.0, 0.0, 0.0);
    else if (fabs(h.x - b.p[3]) < 1e-8) n = v3(1.0, 0.0, 0.0);
    else if (fabs(h.y - b.p[1]) < 1e-8) n = v3(0.0, -1.0, 0.0);
    else if (fabs(h.y - b.p[4]) < 1e-8) n = v3(0.0, 1.0, 0.0);
    else if (fabs(h.z - b.p[2]) < 1e-8) n = v3(0.0, 0.0, -1.0);
    else if (fabs(h.z - b.p[5]) < 1e-8) n = v3(0.0, 0.0, 1.0);
    else { n = v3(1.0, 0.0, 0.0); return false; }
    return true;
}

// Sphere texture coordinates (bodies.rs:126-132).  Kept out of line: the
// f64 atan2/acos expansions need ~70 VGPRs, and inlined into the megakernel
// they set its register peak (247 VGPRs) while every other live value waits.
__device__ __attribute__((noinline)) inline
float2 sphere_uv(double hx, double hy, double hz, double r) {  // returned in VGPRs (no scratch round trip)
    return make_float2((1.0f + ((float)atan2(hz, hx)) / PI_F) * 0.5f, ((float)acos(hy / r)) / PI_F);
}

// bodies.rs:126-132, 155-169, 198-212, 330-333
__device__ __forceinline__ void texture_coords(const RgBodyDev &b, V3 h, float &tx, float &ty) {
    if (b.kind == RG_BODY_SPHERE) {
        V3 hv = sub(h, bp3(b, 0));
        const float2 uv = sphere_uv(hv.x, hv.y, hv.z, b.p[3]);
        tx = uv.x;
        ty = uv.y;
    } else if (b.kind == RG_BODY_AABB) {
        tx = 0.0f;
        ty = 0.0f;
    } else {
        V3 n = bp3(b, 3);
        V3 xa = cross(n, v3(0.0, 0.0, 1.0));
        if (dot(xa, xa) == 0.0) xa = cross(n, v3(0.0, 1.0, 0.0));
        V3 ya = cross(n, xa);
        V3 hv = sub(h, bp3(b, 0));
        tx = (float)dot(hv, xa);
        ty = (float)dot(hv, ya);
    }
}

// material.rs:70-79
__device__ __forceinline__ uint32_t wrap(float v, int32_t max) {
    int32_t w = f32_to_i32(v * (float)max) % max;
    return w < 0 ? (uint32_t)(w + max) : (uint32_t)w;
}

// material.rs:62-68, 82-89 + color.rs:26-30
// (float)b / 255.0f for a byte b (material.rs Texture::color, color.rs from_rgba), correctly
// rounded: one multiply and a residual correction instead of the IEEE division expansion.  Equal to
// the division for every one of the 256 inputs (checked exhaustively: tests/test_primitives_kat.py).
__device__ __forceinline__ float u8_div255(uint32_t b) {
    const float x = (float)b, inv = 1.0f / 255.0f;
    const float q0 = x * inv;
    return __builtin_fmaf(__builtin_fmaf(-q0, 255.0f, x), inv, q0);
}

__device__ __forceinline__ C3 material_color(const RgTexDev *texs, const RgMatDev &m, float tx, float ty) {
    if (m.coloration == RG_COLORATION_COLOR) return c3(m.color[0], m.color[1], m.color[2]);
    const RgTexDev t = texs[m.tex];
    uint32_t x = wrap(tx + m.xoff, t.w);
    uint32_t y = wrap(ty + m.yoff, t.h);
    // texels live in global memory: a global (not flat) load, so its wait does not also drain LDS
    const __attribute__((address_space(1))) uint32_t *tg = (const __attribute__((address_space(1))) uint32_t *)t.texels;
    uint32_t px = tg[(size_t)y * (uint32_t)t.w + x];
    return c3(u8_div255(px & 0xffu), u8_div255((px >> 8) & 0xffu), u8_div255((px >> 16) & 0xffu));
}

// material_color in two halves (light path): the texel load
// is issued at the hit and its conversion runs after the shadow batch's setup, so
// the load's latency overlaps the per-light work instead of stalling the wave.
__device__ __forceinline__ uint32_t texel_fetch(const RgTexDev *texs, const RgMatDev &m, const RgBodyDev &b, V3 h) {
    float tx, ty;
    texture_coords(b, h, tx, ty);
    const RgTexDev t = texs[m.tex];
    uint32_t x = wrap(tx + m.xoff, t.w);
    uint32_t y = wrap(ty + m.yoff, t.h);
    const __attribute__((address_space(1))) uint32_t *tg = (const __attribute__((address_space(1))) uint32_t *)t.texels;
    return tg[(size_t)y * (uint32_t)t.w + x];
}
__device__ __forceinline__ C3 texel_color(uint32_t px) {
    return c3(u8_div255(px & 0xffu), u8_div255((px >> 8) & 0xffu), u8_div255((px >> 16) & 0xffu));
}

// The textured hit of the PLAIN light kernels (no disks, no boxes: a body is a sphere or a plane).
// RG_PLAIN_AXES: a plane's texture axes come from the host's table by body id (RgPlnAxes, rg_exact.h
// rg_plane_axes: the expressions of texture_coords above) -- a subtraction and two dot products
// remain of two cross products, a dot, a compare and a select.  RG_PLAIN_WRAP: material.rs:70-79
// with the texture dimension's magic (RgTexMagic, rg_exact.h rg_wrap_i32) for the i32 % expansion.
// 0: as the other kernels (A/B builds).
#ifndef RG_PLAIN_AXES
#define RG_PLAIN_AXES 1
#endif
#ifndef RG_PLAIN_WRAP
#define RG_PLAIN_WRAP 1
#endif
struct PlainTex {
    const RgTexMagic *texm;  // parallel to the texture descriptors
    const RgPlnAxes *axes;   // by body id
};
__device__ __forceinline__ void texture_coords_plain(const PlainTex &P, const RgBodyDev &b, int id, V3 h, float &tx, float &ty) {
#if RG_PLAIN_AXES
    if (b.kind == RG_BODY_SPHERE) {
        V3 hv = sub(h, bp3(b, 0));
        const float2 uv = sphere_uv(hv.x, hv.y, hv.z, b.p[3]);
        tx = uv.x;
        ty = uv.y;
    } else {
        const RgPlnAxes A = P.axes[id];
        V3 hv = sub(h, bp3(b, 0));
        tx = (float)dot(hv, v3(A.xa[0], A.xa[1], A.xa[2]));
        ty = (float)dot(hv, v3(A.ya[0], A.ya[1], A.ya[2]));
    }
#else
    texture_coords(b, h, tx, ty);
#endif
}
__device__ __forceinline__ uint32_t texel_fetch_plain(const RgTexDev *texs, const PlainTex &P, const RgMatDev &m,
                                                       const RgBodyDev &b, int id, V3 h) {
    float tx, ty;
    texture_coords_plain(P, b, id, h, tx, ty);
    const RgTexDev t = texs[m.tex];
#if RG_PLAIN_WRAP
    const RgTexMagic g = P.texm[m.tex];
    uint32_t x = rg_wrap_i32(f32_to_i32((tx + m.xoff) * (float)t.w), (uint32_t)t.w, g.mw, g.shw);
    uint32_t y = rg_wrap_i32(f32_to_i32((ty + m.yoff) * (float)t.h), (uint32_t)t.h, g.mh, g.shh);
#else
    uint32_t x = wrap(tx + m.xoff, t.w);
    uint32_t y = wrap(ty + m.yoff, t.h);
#endif
    const __attribute__((address_space(1))) uint32_t *tg = (const __attribute__((address_space(1))) uint32_t *)t.texels;
    return tg[(size_t)y * (uint32_t)t.w + x];
}
__device__ __forceinline__ C3 surface_color_plain(const RgTexDev *texs, const PlainTex &P, const RgMatDev &m,
                                                  const RgBodyDev &b, int id, V3 h) {
    if (m.coloration == RG_COLORATION_COLOR) return c3(m.color[0], m.color[1], m.color[2]);
    return texel_color(texel_fetch_plain(texs, P, m, b, id, h));
}

// body.color(&body.texture_coords(hit)) (rendering.rs:134-135, 103).  The
// texture coordinates are pure functions of the hit and only a Texture
// coloration reads them, so they are computed for textured materials only:
// a Color material yields the same colour without the atan2/acos/cross work.
__device__ __forceinline__ C3 surface_color(const RgTexDev *texs, const RgMatDev &m, const RgBodyDev &b, V3 h) {
    if (m.coloration == RG_COLORATION_COLOR) return c3(m.color[0], m.color[1], m.color[2]);
    float tx, ty;
    texture_coords(b, h, tx, ty);
    return material_color(texs, m, tx, ty);
}

// rendering.rs:174-200, `cos_i = cos_t.abs()` (:194) kept as written.
__device__ __forceinline__ double fresnel(V3 inc, V3 n, float index) {
    double i_dot_n = dot(inc, n);
    double eta_i, eta_t;
    if (i_dot_n > 0.0) { eta_i = (double)index; eta_t = 1.0; }
    else { eta_i = 1.0; eta_t = (double)index; }
    double sin_t = eta_i / eta_t * sqrt(fmax(1.0 - i_dot_n * i_dot_n, 0.0));
    if (sin_t > 1.0) return 1.0;
    double cos_t = sqrt(fmax(1.0 - sin_t * sin_t, 0.0));
    double cos_i = fabs(cos_t);
    double r_s = ((eta_t * cos_i) - (eta_i * cos_t)) / ((eta_t * cos_i) + (eta_i * cos_t));
    double r_p = ((eta_i * cos_i) - (eta_t * cos_t)) / ((eta_i * cos_i) + (eta_t * cos_t));
    return (r_s * r_s + r_p * r_p) / 2.0;
}

// ray.rs:56-60
__device__ __forceinline__ Ray reflection(V3 n, V3 inc, V3 h) {
    Ray r;
    r.o = add(h, scl(n, SHADOW_BIAS));
    r.d = sub(inc, scl(n, 2.0 * dot(inc, n)));
    return r;
}

// ray.rs:62-94
__device__ __forceinline__ bool transmission(V3 n, V3 inc, V3 h, float index, Ray &r) {
    V3 ref_n = n;
    double eta_t = (double)index, eta_i = 1.0;
    double i_dot_n = dot(inc, n);
    if (i_dot_n < 0.0) i_dot_n = -i_dot_n;
    else { ref_n = neg(n); eta_t = 1.0; eta_i = (double)index; }
    double eta = eta_i / eta_t;
    double k = 1.0 - (eta * eta) * (1.0 - i_dot_n * i_dot_n);
    if (k < 0.0) return false;
    r.o = add(h, scl(ref_n, -SHADOW_BIAS));
    r.d = sub(scl(add(inc, scl(ref_n, i_dot_n)), eta), scl(ref_n, sqrt(k)));
    return true;
}

// direction_from + distance for one light (lights.rs:46-58).  For a spherical
// light both use |pos - p| = sqrt(dot(v, v)): computed once, same bits.
// U (the PLAIN light kernels, RG_PLAIN_ULIGHT): the square root and the reciprocal without their range
// scaling in the lanes whose operand admits it (rg_k_math.h sqrt_rcp_guarded), same bits.
template <bool U = false>
__device__ __forceinline__ void light_dir_dist(const RgLightDev &l, V3 p, V3 &dir, double &dist) {
    if (l.kind == RG_LIGHT_DIRECTIONAL) {
        dir = v3(l.dn[0], l.dn[1], l.dn[2]);  // normalize(-direction), precomputed
        dist = __builtin_inf();
        return;
    }
    V3 v = sub(v3(l.v[0], l.v[1], l.v[2]), p);
    if constexpr (U) {
        double m, inv;
        sqrt_rcp_guarded(dot(v, v), m, inv);
        dir = scl(v, inv);
        dist = m;
    } else {
        double m = sqrt(dot(v, v));
        dir = scl(v, 1.0 / m);
        dist = m;
    }
}

// lights.rs:46-58
__device__ __forceinline__ V3 light_dir(const RgLightDev &l, V3 p) {
    if (l.kind == RG_LIGHT_DIRECTIONAL) return v3(l.dn[0], l.dn[1], l.dn[2]);  // normalize(-dir), precomputed
    return normalize(sub(v3(l.v[0], l.v[1], l.v[2]), p));
}
__device__ __forceinline__ double light_distance(const RgLightDev &l, V3 p) {
    if (l.kind == RG_LIGHT_DIRECTIONAL) return __builtin_inf();
    V3 d = sub(v3(l.v[0], l.v[1], l.v[2]), p);
    return sqrt(dot(d, d));
}
__device__ __forceinline__ float light_intensity(const RgLightDev &l, V3 p) {  // lights.rs:36-44
    if (l.kind == RG_LIGHT_DIRECTIONAL) return l.intensity;
    V3 d = sub(v3(l.v[0], l.v[1], l.v[2]), p);
    float r2 = (float)dot(d, d);
    return l.intensity / (4.0f * PI_F * r2);
}

}  // namespace rgk
