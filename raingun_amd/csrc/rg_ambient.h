// rg_ambient.h — the ambient term's arithmetic, said once (the text is in include/raingun.h at
// rg_ao_filter and rg_render_image_ambient).  No HIP include: the kernels (rg_ao_filter.hip), the host (the
// entry points' validation, the scene's share table) and the stand-alone CPU test (tests/native/ambient_test.cpp)
// share it, as they share rg_ao.h.
//
// 1. The edge-stopping filter of the AO pass.  Per pixel p = (x, y) with b = body[p], n_p = normal[p], radius r,
//    f32, unfused, in this order:
//        b < 0:  out[p] = ao[p]
//        nn_p = (n_p.x*n_p.x + n_p.y*n_p.y) + n_p.z*n_p.z;  t = normal_min * normal_min
//        sum = 0.0f;  wsum = 0
//        for dy = -r .. r, for dx = -r .. r, q = (x + dx, y + dy) inside the frame:
//            w = (r + 1 - |dx|) * (r + 1 - |dy|)
//            d = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z
//            accepted iff q == p, or body[q] == b && d > 0.0f && d*d >= t * (nn_p * nn_q)
//            accepted:  sum = sum + (float)w * ao[q];  wsum += w
//        out[p] = sum / (float)wsum
// 2. share[b], one f32 per body: diffuse albedo; reflecting (1.0f - reflectivity) * albedo; refractive 0.0f.
// 3. The compose, per pixel and channel c:  hit: v = rgb.c + (color.c * albedo.c) * (share[b] * aof);  miss: v = rgb.c;
//    v clamped as a sample; the byte is (u8)(v * 255.0f).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define RG_AMBIENT_FN __host__ __device__ __forceinline__
#else
#define RG_AMBIENT_FN inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define RG_AO_FILTER_MAX_RADIUS 8u

// May {radius, normal_min} be a filter?  radius 1 .. 8; normal_min in [0, 1] (a NaN fails both comparisons).
RG_AMBIENT_FN bool rg_ao_filter_valid(uint32_t radius, float normal_min) {
    return radius >= 1u && radius <= RG_AO_FILTER_MAX_RADIUS && normal_min >= 0.0f && normal_min <= 1.0f;
}

// May these be an ambient term?  colour finite and >= 0, samples 1 .. 8, filter_radius 0 .. 8 (0: unfiltered),
// normal_min in [0, 1].  (The AO pass is rg_ao_valid's.)
RG_AMBIENT_FN bool rg_ambient_valid(const float color[3], uint32_t samples, uint32_t filter_radius, float normal_min) {
    for (int c = 0; c < 3; ++c)
        if (!(color[c] >= 0.0f) || color[c] - color[c] != 0.0f) return false;
    return samples >= 1u && samples <= 8u && filter_radius <= RG_AO_FILTER_MAX_RADIUS && normal_min >= 0.0f &&
           normal_min <= 1.0f;
}

// n . n and a . b, in the contract's order.
RG_AMBIENT_FN float rg_ambient_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

// The tent's weight of tap (dx, dy): an integer <= 81.
RG_AMBIENT_FN int rg_ao_filter_weight(int r, int dx, int dy) {
    return (r + 1 - (dx < 0 ? -dx : dx)) * (r + 1 - (dy < 0 ? -dy : dy));
}

// Is the tap q, not the centre, accepted by centre p?  d = n_p . n_q; t = normal_min^2.  A NaN compares false.
RG_AMBIENT_FN bool rg_ao_filter_accepts(int32_t body_p, int32_t body_q, float d, float nn_p, float nn_q, float t) {
    return body_q == body_p && d > 0.0f && d * d >= t * (nn_p * nn_q);
}

// One pixel of the filter from whole-frame layers, on the host.  The library does not call it: the kernel walks the
// same taps in the same order from its LDS tile with the predicates, the weight and the dot product above, and this
// is the loop around them for a stand-alone program (tests/native/ambient_test.cpp) to run.
inline float rg_ao_filter_pixel(const float *ao, const int32_t *body, const float *normal, uint32_t width,
                                uint32_t height, uint32_t radius, float normal_min, uint32_t x, uint32_t y) {
    const size_t p = (size_t)y * width + x;
    const int32_t b = body[p];
    if (b < 0) return ao[p];
    const float *np = normal + 3 * p;
    const float nn_p = rg_ambient_dot(np[0], np[1], np[2], np[0], np[1], np[2]);
    const float t = normal_min * normal_min;
    const int r = (int)radius;
    float sum = 0.0f;
    int wsum = 0;
    for (int dy = -r; dy <= r; ++dy)
        for (int dx = -r; dx <= r; ++dx) {
            const long long qx = (long long)x + dx, qy = (long long)y + dy;
            if (qx < 0 || qy < 0 || qx >= (long long)width || qy >= (long long)height) continue;
            const size_t q = (size_t)qy * width + (size_t)qx;
            const float *nq = normal + 3 * q;
            const float d = rg_ambient_dot(np[0], np[1], np[2], nq[0], nq[1], nq[2]);
            const float nn_q = rg_ambient_dot(nq[0], nq[1], nq[2], nq[0], nq[1], nq[2]);
            if (q == p || rg_ao_filter_accepts(b, body[q], d, nn_p, nn_q, t)) {
                const int w = rg_ao_filter_weight(r, dx, dy);
                sum = sum + (float)w * ao[q];
                wsum += w;
            }
        }
    return sum / (float)wsum;
}

// share[b] of a body's material (surface: rg_surface_kind of include/raingun.h).
RG_AMBIENT_FN float rg_ambient_share(uint32_t surface, float albedo, float reflectivity) {
    if (surface == 0u) return albedo;
    if (surface == 1u) return (1.0f - reflectivity) * albedo;
    return 0.0f;
}

// A sample's clamp (rg_resolve.hip): s if 0 <= s <= 1, 1 if s > 1, else 0 (negatives and NaN).
RG_AMBIENT_FN float rg_ambient_clamp(float s) { return (s >= 0.0f && s <= 1.0f) ? s : (s > 1.0f ? 1.0f : 0.0f); }

// One channel of the composed pixel, clamped.  hit: body >= 0.
RG_AMBIENT_FN float rg_ambient_channel(float rgb, float color, float albedo, float share, float aof, bool hit) {
    return rg_ambient_clamp(hit ? rgb + (color * albedo) * (share * aof) : rgb);
}

// Rust `f32 as u8` of v * 255: truncate, saturate, NaN -> 0.
RG_AMBIENT_FN uint32_t rg_ambient_u8(float v) {
    const float s = v * 255.0f;
    if (!(s > 0.0f)) return 0u;
    if (s >= 255.0f) return 255u;
    return (uint32_t)s;
}
