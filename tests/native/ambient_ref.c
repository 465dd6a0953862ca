/* ambient_ref.c -- the reference of the ambient term's tests (tests/ambient_ref.py): the edge-stopping filter of
 * the AO pass, the per-body share and the compose, written from the text of include/raingun.h (rg_ao_filter,
 * rg_render_image_ambient) and from nothing else of the library.  Plain C, f32, built with the oracle's compiler
 * and flags (contraction off).  Test-side only. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/raingun.h"

static float dot3(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

static int iabs(int v) { return v < 0 ? -v : v; }

/* Is tap q (not the centre) accepted by centre p? */
static int accepted(const int32_t *body, const float *normal, size_t p, size_t q, float t) {
    const float *np = normal + 3 * p, *nq = normal + 3 * q;
    const float nn_p = dot3(np, np), nn_q = dot3(nq, nq);
    const float d = dot3(np, nq);
    return body[q] == body[p] && d > 0.0f && d * d >= t * (nn_p * nn_q);
}

/* out = the filter of ao.  reverse != 0: the taps in the opposite order (NOT the contract: the tests use it to show
 * that the order is observable). */
void amb_filter(const float *ao, const int32_t *body, const float *normal, uint32_t width, uint32_t height, uint32_t radius,
                float normal_min, int32_t reverse, float *out) {
    const int r = (int)radius, side = 2 * r + 1, taps = side * side;
    const float t = normal_min * normal_min;
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const size_t p = (size_t)y * width + x;
            if (body[p] < 0) {
                out[p] = ao[p];
                continue;
            }
            float sum = 0.0f;
            int wsum = 0;
            for (int i = 0; i < taps; ++i) {
                const int k = reverse ? taps - 1 - i : i;
                const int dy = k / side - r, dx = k % side - r; /* dy outer, dx inner */
                const int64_t qx = (int64_t)x + dx, qy = (int64_t)y + dy;
                if (qx < 0 || qy < 0 || qx >= (int64_t)width || qy >= (int64_t)height) continue;
                const size_t q = (size_t)qy * width + (size_t)qx;
                if (!((dx == 0 && dy == 0) || accepted(body, normal, p, q, t))) continue;
                const int w = (r + 1 - iabs(dx)) * (r + 1 - iabs(dy));
                sum = sum + (float)w * ao[q];
                wsum += w;
            }
            out[p] = sum / (float)wsum;
        }
}

/* What the guides do to the filter, for the tests' conditions on their inputs: over hit pixels p (body >= 0) and
 * their in-frame taps q != p, pairs[0] += the pairs, pairs[1] += the accepted ones; rejecting[p] = 1 if some
 * in-frame tap of p is rejected, else 0 (0 for a miss). */
void amb_pairs(const int32_t *body, const float *normal, uint32_t width, uint32_t height, uint32_t radius, float normal_min,
               uint64_t pairs[2], uint8_t *rejecting) {
    const int r = (int)radius;
    const float t = normal_min * normal_min;
    pairs[0] = pairs[1] = 0;
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const size_t p = (size_t)y * width + x;
            rejecting[p] = 0;
            if (body[p] < 0) continue;
            for (int dy = -r; dy <= r; ++dy)
                for (int dx = -r; dx <= r; ++dx) {
                    const int64_t qx = (int64_t)x + dx, qy = (int64_t)y + dy;
                    if ((dx == 0 && dy == 0) || qx < 0 || qy < 0 || qx >= (int64_t)width || qy >= (int64_t)height) continue;
                    const int ok = accepted(body, normal, p, (size_t)qy * width + (size_t)qx, t);
                    pairs[0] += 1;
                    pairs[1] += (uint64_t)ok;
                    if (!ok) rejecting[p] = 1;
                }
        }
}

/* share[b] for every body of the description. */
void amb_shares(const rg_scene_desc *d, float *share) {
    for (uint32_t b = 0; b < d->n_bodies; ++b) {
        const rg_material *m = &d->bodies[b].material;
        if (m->surface == RG_SURFACE_DIFFUSE) share[b] = m->albedo;
        else if (m->surface == RG_SURFACE_REFLECTING) share[b] = (1.0f - m->reflectivity) * m->albedo;
        else share[b] = 0.0f;
    }
}

static float clamp_sample(float v) { return (v >= 0.0f && v <= 1.0f) ? v : (v > 1.0f ? 1.0f : 0.0f); }

/* `f32 as u8`: truncate, saturate, NaN -> 0 (color.rs:32-37) */
static uint8_t as_u8(float v) {
    if (!(v > 0.0f)) return 0;
    if (v >= 255.0f) return 255;
    return (uint8_t)v;
}

/* The compose over npx pixels: rgb_out (npx x 3) the clamped v, rgba (npx x 4) the bytes. */
void amb_compose(const float *rgb, const float *albedo, const int32_t *body, const float *aof, const float *share,
                 const float color[3], uint64_t npx, float *rgb_out, uint8_t *rgba) {
    for (uint64_t p = 0; p < npx; ++p) {
        const int32_t b = body[p];
        for (int c = 0; c < 3; ++c) {
            float v = rgb[3 * p + c];
            if (b >= 0) v = rgb[3 * p + c] + (color[c] * albedo[3 * p + c]) * (share[b] * aof[p]);
            v = clamp_sample(v);
            rgb_out[3 * p + c] = v;
            rgba[4 * p + c] = as_u8(v * 255.0f);
        }
        rgba[4 * p + 3] = 255;
    }
}
