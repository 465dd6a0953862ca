// rg_camera.h — the movable camera's arithmetic, said once.  No HIP include: the
// render kernels (rg_render_kernel.h, the RGR_PRIM site of the camera family), the host
// (rg_camera_look_at, rg_scene_set_camera) and the stand-alone CPU test
// (tests/native/camera_test.cpp) share it, as they share rg_exact.h and rg_tile_deal.h.
//
// A camera is eye, right, up, forward: four triples of doubles, all finite, forward not all
// zero.  For pixel (x, y) of a w x h frame, with the reference's sensor coordinates sx, sy
// (ray.rs:43-51):
//     D.k = (right.k * sx + up.k * sy) + forward.k          k = x, y, z; f64, this order, no FMA
//     ray = Ray::new(eye, normalize(D))                     normalize: v * (1 / |v|), |v|^2 = (x.x + y.y) + z.z
// With eye = 0, right = (1,0,0), up = (0,1,0), forward = (0,0,-1) that is the reference's
// create_prime bit for bit: 1 * sx and 1 * sy are exact, sx and sy are never -0, +0 + (+-0) = +0,
// 0 * s + 0 * s = +0 and +0 + -1 = -1.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define RG_CAMERA_FN __host__ __device__ __forceinline__
#else
#define RG_CAMERA_FN inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// The reference's sensor coordinates of pixel (x, y) (ray.rs:43-51): the expressions of
// rg_k_math.h sensor_div and of the oracle's create_prime.  width_d, height_d: the frame size as
// doubles; aspect = width_d / height_d; fov_adjustment = tan(fov.to_radians() / 2).
RG_CAMERA_FN void rg_camera_sensor(uint32_t x, uint32_t y, double width_d, double height_d, double aspect,
                                   double fov_adjustment, double *sx, double *sy) {
    *sx = ((((double)x + 0.5) / width_d) * 2.0 - 1.0) * aspect * fov_adjustment;
    *sy = (1.0 - (((double)y + 0.5) / height_d) * 2.0) * fov_adjustment;
}

// The project's normalize: v * (1 / |v|), dot order (x.x + y.y) + z.z.
RG_CAMERA_FN void rg_camera_normalize(const double v[3], double out[3]) {
    const double inv = 1.0 / sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    out[0] = v[0] * inv;
    out[1] = v[1] * inv;
    out[2] = v[2] * inv;
}

// The direction of the camera ray through sensor point (sx, sy).
RG_CAMERA_FN void rg_camera_direction(const double right[3], const double up[3], const double forward[3], double sx,
                                      double sy, double dir[3]) {
    double d[3];
    d[0] = (right[0] * sx + up[0] * sy) + forward[0];
    d[1] = (right[1] * sx + up[1] * sy) + forward[1];
    d[2] = (right[2] * sx + up[2] * sy) + forward[2];
    rg_camera_normalize(d, dir);
}

RG_CAMERA_FN void rg_camera_cross(const double a[3], const double b[3], double out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

RG_CAMERA_FN bool rg_camera_finite3(const double v[3]) {
    // (x - x is 0 for every finite x, NaN for NaN and the infinities)
    return v[0] - v[0] == 0.0 && v[1] - v[1] == 0.0 && v[2] - v[2] == 0.0;
}

// May this basis be a camera?  Every member finite, forward not all zero.
RG_CAMERA_FN bool rg_camera_valid(const double eye[3], const double right[3], const double up[3],
                                  const double forward[3]) {
    return rg_camera_finite3(eye) && rg_camera_finite3(right) && rg_camera_finite3(up) && rg_camera_finite3(forward) &&
           !(forward[0] == 0.0 && forward[1] == 0.0 && forward[2] == 0.0);
}

// look_at: f = normalize(target - eye), r = normalize(cross(f, up_hint)), u = cross(r, f).
// false (nothing written) for target == eye, a non-finite input, cross(f, up_hint) == 0, or a
// result that is no camera (an overflow on the way).
RG_CAMERA_FN bool rg_camera_look_at_basis(const double eye[3], const double target[3], const double up_hint[3],
                                          double right[3], double up[3], double forward[3]) {
    if (!rg_camera_finite3(eye) || !rg_camera_finite3(target) || !rg_camera_finite3(up_hint)) return false;
    if (target[0] == eye[0] && target[1] == eye[1] && target[2] == eye[2]) return false;
    const double t[3] = {target[0] - eye[0], target[1] - eye[1], target[2] - eye[2]};
    double f[3], c[3], r[3], u[3];
    rg_camera_normalize(t, f);
    rg_camera_cross(f, up_hint, c);
    if (c[0] == 0.0 && c[1] == 0.0 && c[2] == 0.0) return false;
    rg_camera_normalize(c, r);
    rg_camera_cross(r, f, u);
    if (!rg_camera_valid(eye, r, u, f)) return false;
    for (int k = 0; k < 3; ++k) {
        right[k] = r[k];
        up[k] = u[k];
        forward[k] = f[k];
    }
    return true;
}
