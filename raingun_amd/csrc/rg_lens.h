// rg_lens.h — the thin lens's arithmetic, said once.  No HIP include: the render
// kernels (rg_render_kernel.h, the RGR_PRIM site of the lens family), the host (rg_scene_set_lens,
// rg_lens_tables, the launch's LR / LU) and the stand-alone CPU test (tests/native/lens_test.cpp)
// share it, as they share rg_camera.h, on which it stands.
//
// A lens is aperture (the lens radius, world units) and focus (the distance of the plane in focus
// along forward, in units of |forward|).  It applies to the k x k samples per pixel of a supersampled
// frame, k >= 2.  For pixel (X, Y) of the kW x kH sample frame, with the camera (E, R, U, F) and the
// sensor coordinates sx, sy of rg_camera_sensor -- f64, unfused, in this order:
//     D.c  = (R.c * sx + U.c * sy) + F.c                     rg_camera_direction before its normalize
//     s    = (Y % k) * k + (X % k)                            the sample's lens point (pu, pv) = points_k[s]
//     n    = (Y / k) * W + (X / k)                            the output pixel; h = rg_lens_hash(n)
//     (c, g) = rotations[h & 63]                              the pixel's turn of the lens disk
//     qu = c * pu - g * pv;  qv = g * pu + c * pv
//     O.c  = LR.c * qu + LU.c * qv                            LR = normalize(R) * aperture, LU = normalize(U) * aperture
//     origin.c = E.c + O.c
//     V.c  = D.c * focus - O.c
//     ray  = Ray::new(origin, normalize(V))                   rg_camera_normalize
// The two tables are made on the host (rg_lens_make_tables) and travel as doubles: no transcendental
// is evaluated where rays are made.
#pragma once
#include "rg_camera.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define RG_LENS_MAX_SAMPLES 8   // k = 1 .. 8 (RG_AA_MAX_SAMPLES)
#define RG_LENS_POINTS 204      // 1 + 4 + 9 + .. + 64 points, k's at rg_lens_points_offset(k)
#define RG_LENS_ROTATIONS 64
// one table: the points of every k (2 doubles each), then the rotations (cos, sin)
#define RG_LENS_TABLE_DOUBLES (2 * RG_LENS_POINTS + 2 * RG_LENS_ROTATIONS)

// lowbias32: the hash of the output pixel's index that picks its turn of the lens disk.
RG_CAMERA_FN uint32_t rg_lens_hash(uint32_t n) {
    n ^= n >> 16;
    n *= 0x7feb352du;
    n ^= n >> 15;
    n *= 0x846ca68bu;
    n ^= n >> 16;
    return n;
}

// Points in front of k's in the table: 1 + 4 + .. + (k - 1)^2.
RG_CAMERA_FN uint32_t rg_lens_points_offset(uint32_t k) { return (k - 1u) * k * (2u * k - 1u) / 6u; }

// May {aperture, focus} be a lens?  Both finite, aperture >= 0, focus > 0.
RG_CAMERA_FN bool rg_lens_valid(double aperture, double focus) {
    return aperture - aperture == 0.0 && focus - focus == 0.0 && aperture >= 0.0 && focus > 0.0;
}

// Does a frame of samples x samples rays per pixel see the lens?  Not with aperture == 0 (a pinhole)
// and not with one sample per pixel: those frames are the ones the scene renders without a lens.
RG_CAMERA_FN bool rg_lens_active(double aperture, uint32_t samples) { return aperture > 0.0 && samples >= 2u; }

// LR or LU: normalize(axis) * aperture.
RG_CAMERA_FN void rg_lens_axis(const double axis[3], double aperture, double out[3]) {
    double n[3];
    rg_camera_normalize(axis, n);
    out[0] = n[0] * aperture;
    out[1] = n[1] * aperture;
    out[2] = n[2] * aperture;
}

// The lens ray of sample-frame pixel (x, y), whose sensor coordinates are (sx, sy): k x k samples per
// pixel of a frame `out_w` output pixels wide.  points_k: k's points, rotations: the 64 turns.
RG_CAMERA_FN void rg_lens_ray(const double eye[3], const double right[3], const double up[3], const double forward[3],
                              double sx, double sy, uint32_t x, uint32_t y, uint32_t k, uint32_t out_w, double focus,
                              const double lr[3], const double lu[3], const double *points_k, const double *rotations,
                              double origin[3], double dir[3]) {
    const uint32_t s = (y % k) * k + (x % k);
    const uint32_t h = rg_lens_hash((y / k) * out_w + (x / k));
    const double pu = points_k[2u * s], pv = points_k[2u * s + 1u];
    const double c = rotations[2u * (h & 63u)], g = rotations[2u * (h & 63u) + 1u];
    const double qu = c * pu - g * pv, qv = g * pu + c * pv;
    double v[3];
    for (int i = 0; i < 3; ++i) {
        const double d = (right[i] * sx + up[i] * sy) + forward[i];
        const double o = lr[i] * qu + lu[i] * qv;
        origin[i] = eye[i] + o;
        v[i] = d * focus - o;
    }
    rg_camera_normalize(v, dir);
}

// Host only (libm), from here on.
// The concentric (Shirley-Chiu) map of the unit square's (u, v) onto the unit disk; the centre exactly (0, 0).
inline void rg_lens_concentric(double u, double v, double *px, double *py) {
    const double quarter_pi = 0.78539816339744830962, half_pi = 1.57079632679489661923;
    const double a = 2.0 * u - 1.0, b = 2.0 * v - 1.0;
    if (a == 0.0 && b == 0.0) {
        *px = 0.0;
        *py = 0.0;
        return;
    }
    double r, phi;
    if (fabs(a) > fabs(b)) {
        r = a;
        phi = quarter_pi * (b / a);
    } else {
        r = b;
        phi = half_pi - quarter_pi * (a / b);
    }
    *px = r * cos(phi);
    *py = r * sin(phi);
}

// k's points: the map of the cell centres ((i + 0.5) / k, (j + 0.5) / k) of the k x k grid, at index j * k + i.
inline void rg_lens_make_points(uint32_t k, double *points) {
    for (uint32_t j = 0; j < k; ++j)
        for (uint32_t i = 0; i < k; ++i)
            rg_lens_concentric(((double)i + 0.5) / (double)k, ((double)j + 0.5) / (double)k, &points[2u * (j * k + i)],
                               &points[2u * (j * k + i) + 1u]);
}

// rotations[m] = (cos, sin) of 2 pi m / 64.
inline void rg_lens_make_rotations(double *rotations) {
    const double two_pi = 6.28318530717958647692;
    for (uint32_t m = 0; m < RG_LENS_ROTATIONS; ++m) {
        const double t = two_pi * (double)m / (double)RG_LENS_ROTATIONS;
        rotations[2u * m] = cos(t);
        rotations[2u * m + 1u] = sin(t);
    }
}

// The whole table (RG_LENS_TABLE_DOUBLES doubles), as the device holds it.
inline void rg_lens_make_tables(double *table) {
    for (uint32_t k = 1; k <= RG_LENS_MAX_SAMPLES; ++k) rg_lens_make_points(k, table + 2u * rg_lens_points_offset(k));
    rg_lens_make_rotations(table + 2u * RG_LENS_POINTS);
}
