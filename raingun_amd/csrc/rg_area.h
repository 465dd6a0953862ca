// rg_area.h — the area lights' arithmetic, said once.  No HIP include: the render kernels
// (rg_render_kernel.h, the light_at helper of the area family), the host (rg_scene_set_light_radii,
// rg_area_tables, the device table) and the stand-alone CPU test (tests/native/area_test.cpp) share it, as
// they share rg_lens.h, on whose hash, rotations and table offsets it stands.
//
// A spherical light l has a radius radius[l] >= 0 (world units; a directional light's is 0).  It applies to
// the k x k samples per pixel of a supersampled frame, k >= 2.  For pixel (X, Y) of the kW x kH sample frame
// (Y the row of the whole frame) and the light of index l, with the light's centre v -- u32 wrap-around,
// then f64, unfused, in this order:
//     s = (Y % k) * k + (X % k)                      the sample
//     n = (Y / k) * W + (X / k)                      the output pixel
//     g = rg_lens_hash(n ^ ((l + 1) * 0x9e3779b9))
//     j = (s + (g >> 6)) % (k * k)                   this pixel's and light's shift through the points
//     (c, e) = rotations[g & 63]                     the lens's 64 turns, here about world z
//     (px, py, pz) = sphere_points_k[j]
//     qx = c * px - e * py;  qy = e * px + c * py;  qz = pz
//     position.c = v.c + radius[l] * q.c             radius 0 included
// Everything the sample's ray tree does with the light's position uses `position`.  The points are made on
// the host (rg_area_make_points) and travel as doubles: no transcendental is evaluated where rays are made.
#pragma once
#include "rg_lens.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define RG_AREA_KEY 0x9e3779b9u
// the device table: the points of every k = 1 .. 8 (3 doubles each, k's at rg_lens_points_offset(k)),
// then the scene's radii, one per light
#define RG_AREA_POINT_DOUBLES (3 * RG_LENS_POINTS)
RG_CAMERA_FN uint32_t rg_area_table_doubles(uint32_t n_lights) { return RG_AREA_POINT_DOUBLES + n_lights; }

// May r be a light's radius?  Finite and >= 0.
RG_CAMERA_FN bool rg_area_radius_valid(double r) { return r - r == 0.0 && r >= 0.0; }

// Does a frame of samples x samples rays per pixel see the radii?  Not with every radius 0 (point lights)
// and not with one sample per pixel: those frames are the ones the scene renders without radii.
RG_CAMERA_FN bool rg_area_active(bool any_radius, uint32_t samples) { return any_radius && samples >= 2u; }

// The index j of the sample's point and the index m of its turn: pixel (x, y) of the sample frame, k x k
// samples per pixel of a frame `out_w` output pixels wide, light l.
RG_CAMERA_FN void rg_area_index(uint32_t x, uint32_t y, uint32_t k, uint32_t out_w, uint32_t l, uint32_t *j, uint32_t *m) {
    const uint32_t s = (y % k) * k + (x % k);
    const uint32_t n = (y / k) * out_w + (x / k);
    const uint32_t g = rg_lens_hash(n ^ ((l + 1u) * RG_AREA_KEY));
    *j = (s + (g >> 6)) % (k * k);
    *m = g & 63u;
}

// The position of light l (centre v, radius r) as that sample sees it.  points_k: k's points (3 doubles
// each), rotations: the lens's 64 turns.
RG_CAMERA_FN void rg_area_position(const double v[3], double r, uint32_t x, uint32_t y, uint32_t k, uint32_t out_w,
                                   uint32_t l, const double *points_k, const double *rotations, double pos[3]) {
    uint32_t j, m;
    rg_area_index(x, y, k, out_w, l, &j, &m);
    const double px = points_k[3u * j], py = points_k[3u * j + 1u], pz = points_k[3u * j + 2u];
    const double c = rotations[2u * m], e = rotations[2u * m + 1u];
    const double qx = c * px - e * py, qy = e * px + c * py;
    pos[0] = v[0] + r * qx;
    pos[1] = v[1] + r * qy;
    pos[2] = v[2] + r * pz;
}

// Host only (libm), from here on.
// k's points: cell (i, j) of the k x k grid, at index j * k + i, mapped onto the unit sphere --
// u = (i + 0.5) / k, v = (j + 0.5) / k; z = 1 - 2u, rho = sqrt(1 - z z), phi = 2 pi v (uniform in area).
inline void rg_area_make_points(uint32_t k, double *points) {
    const double two_pi = 6.28318530717958647692;
    for (uint32_t j = 0; j < k; ++j)
        for (uint32_t i = 0; i < k; ++i) {
            const double u = ((double)i + 0.5) / (double)k, v = ((double)j + 0.5) / (double)k;
            const double z = 1.0 - 2.0 * u, rho = sqrt(1.0 - z * z), phi = two_pi * v;
            double *p = points + 3u * (j * k + i);
            p[0] = rho * cos(phi);
            p[1] = rho * sin(phi);
            p[2] = z;
        }
}

// The points of the whole table (RG_AREA_POINT_DOUBLES doubles), as the device holds them in front of the radii.
inline void rg_area_make_table_points(double *table) {
    for (uint32_t k = 1; k <= RG_LENS_MAX_SAMPLES; ++k) rg_area_make_points(k, table + 3u * rg_lens_points_offset(k));
}
