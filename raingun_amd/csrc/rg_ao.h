// rg_ao.h — the ambient occlusion pass's arithmetic, said once.  No HIP include: the kernel
// (rg_ao_kernel.h), the host (rg_ao_tables, the device table, the entry points' validation) and the
// stand-alone CPU test (tests/native/ao_test.cpp) share it, as they share rg_lens.h, on whose hash,
// points, rotations and table offsets it stands.
//
// An AO pass is {samples = k, radius, bias}.  For pixel (x, y) of a `width` pixels wide frame whose primary
// ray (o, d) hit a body at distance t, with n the reference's surface_normal there -- f64, unfused, in this
// order:
//     h    = o + d * t
//     m    = normalize(n);  nf = dot(m, d) <= 0 ? m : -m              the side the ray came from
//     O.c  = h.c + nf.c * bias
//     s    = copysign(1, nf.z);  a = -1 / (s + nf.z);  b = (nf.x * nf.y) * a       (Duff et al.)
//     T    = (1 + (s * nf.x) * (nf.x * a),  s * b,  (-s) * nf.x)
//     B    = (b,  s + (nf.y * nf.y) * a,  -nf.y)
//     (c, g) = rotations[rg_lens_hash(y * width + x) & 63]             the pixel's turn about nf
//     Tr.c = c * T.c + g * B.c;  Br.c = c * B.c - g * T.c
//     D.c  = (Tr.c * px + Br.c * py) + nf.c * pz                        (px, py, pz) = ao_points_k[j], j = 0 .. k^2 - 1
//     ray  = Ray::new(O, normalize(D));  occluded iff Scene::trace hits with !(t > radius)
//     ao   = (float)open / (float)(k * k)
// The points are made on the host (rg_ao_make_points) and travel as doubles: no transcendental is evaluated
// where rays are made.
#pragma once
#include "rg_lens.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define RG_AO_MAX_SAMPLES RG_LENS_MAX_SAMPLES
// the device table: the points of every k = 1 .. 8 (3 doubles each, k's at rg_lens_points_offset(k)), then the
// lens's 64 rotations (cos, sin)
#define RG_AO_POINT_DOUBLES (3 * RG_LENS_POINTS)
#define RG_AO_TABLE_DOUBLES (RG_AO_POINT_DOUBLES + 2 * RG_LENS_ROTATIONS)

// May {samples, radius, bias} be an AO pass?  samples 1 .. 8; radius > 0, +inf allowed; bias finite and >= 0.
RG_CAMERA_FN bool rg_ao_valid(uint32_t samples, double radius, double bias) {
    return samples >= 1u && samples <= RG_AO_MAX_SAMPLES && radius > 0.0 && bias - bias == 0.0 && bias >= 0.0;
}

// nf: the unit normal on the side the ray of direction d came from.
RG_CAMERA_FN void rg_ao_facing(const double n[3], const double d[3], double nf[3]) {
    double m[3];
    rg_camera_normalize(n, m);
    const bool keep = (m[0] * d[0] + m[1] * d[1]) + m[2] * d[2] <= 0.0;
    nf[0] = keep ? m[0] : -m[0];
    nf[1] = keep ? m[1] : -m[1];
    nf[2] = keep ? m[2] : -m[2];
}

// The origin of the pixel's AO rays.
RG_CAMERA_FN void rg_ao_origin(const double h[3], const double nf[3], double bias, double o[3]) {
    o[0] = h[0] + nf[0] * bias;
    o[1] = h[1] + nf[1] * bias;
    o[2] = h[2] + nf[2] * bias;
}

// The tangent frame (T, B) of the unit vector nf: branch-free, no square root, defined for every nf
// (nf.z = -0.0 takes s = -1).
RG_CAMERA_FN void rg_ao_frame(const double nf[3], double t[3], double bt[3]) {
    const double s = copysign(1.0, nf[2]);
    const double a = -1.0 / (s + nf[2]);
    const double b = (nf[0] * nf[1]) * a;
    t[0] = 1.0 + (s * nf[0]) * (nf[0] * a);
    t[1] = s * b;
    t[2] = (-s) * nf[0];
    bt[0] = b;
    bt[1] = s + (nf[1] * nf[1]) * a;
    bt[2] = -nf[1];
}

// The frame turned about nf by (c, g) = (cos, sin).
RG_CAMERA_FN void rg_ao_turn(const double t[3], const double bt[3], double c, double g, double tr[3], double br[3]) {
    for (int i = 0; i < 3; ++i) {
        tr[i] = c * t[i] + g * bt[i];
        br[i] = c * bt[i] - g * t[i];
    }
}

// The pixel's turn: (c, g) of pixel p = y * width + x.
RG_CAMERA_FN uint32_t rg_ao_turn_index(uint32_t pixel) { return rg_lens_hash(pixel) & 63u; }

// The direction of the ray through point (px, py, pz) of the hemisphere, normalised.
RG_CAMERA_FN void rg_ao_direction(const double tr[3], const double br[3], const double nf[3], double px, double py,
                                  double pz, double dir[3]) {
    double d[3];
    d[0] = (tr[0] * px + br[0] * py) + nf[0] * pz;
    d[1] = (tr[1] * px + br[1] * py) + nf[1] * pz;
    d[2] = (tr[2] * px + br[2] * py) + nf[2] * pz;
    rg_camera_normalize(d, dir);
}

// Host only (libm), from here on.
// k's points: the lens's point (pu, pv) of index j * k + i lifted onto the unit hemisphere (Malley: a
// uniform disk gives cosine-weighted directions).
inline void rg_ao_make_points(uint32_t k, double *points) {
    double disk[2 * RG_LENS_MAX_SAMPLES * RG_LENS_MAX_SAMPLES];
    rg_lens_make_points(k, disk);
    for (uint32_t j = 0; j < k * k; ++j) {
        const double pu = disk[2u * j], pv = disk[2u * j + 1u];
        points[3u * j] = pu;
        points[3u * j + 1u] = pv;
        points[3u * j + 2u] = sqrt(fmax(0.0, (1.0 - pu * pu) - pv * pv));
    }
}

// The whole table (RG_AO_TABLE_DOUBLES doubles), as the device holds it.
inline void rg_ao_make_table(double *table) {
    for (uint32_t k = 1; k <= RG_AO_MAX_SAMPLES; ++k) rg_ao_make_points(k, table + 3u * rg_lens_points_offset(k));
    rg_lens_make_rotations(table + RG_AO_POINT_DOUBLES);
}
