// camera_test.cpp — raingun_amd/csrc/rg_camera.h on the CPU (tests/test_camera_cpu.py builds and runs it).
//   * identity camera: the ray of every pixel at 1x1, 17x3, 97x61 and 64x48 has the bits of the
//     reference's create_prime expressions (ray.rs:37-54), origin +0 included
//   * look_at(0, (0,0,-1), (0,1,0)) is a camera whose rays equal the identity camera's
//   * look_at results are orthonormal to 4 ulp of 1.0 for a handful of poses
//   * each rejected input is rejected, and leaves its outputs alone
//   * `look_at ex ey ez tx ty tz ux uy uz` prints the basis as 9 hex doubles (or "rejected"), for the
//     comparison with raingun_amd.camera.Camera.look_at
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../raingun_amd/csrc/rg_camera.h"

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static uint64_t bits(double v) {
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

static const double kEye0[3] = {0.0, 0.0, 0.0}, kRight[3] = {1.0, 0.0, 0.0}, kUp[3] = {0.0, 1.0, 0.0},
                    kFwd[3] = {0.0, 0.0, -1.0};

// create_prime as the reference writes it (and oracle/raingun_oracle.c restates it)
static void create_prime(uint32_t x, uint32_t y, uint32_t w, uint32_t h, double fov_adj, double o[3], double d[3]) {
    const double aspect = (double)w / (double)h;
    const double sx = ((((double)x + 0.5) / (double)w) * 2.0 - 1.0) * aspect * fov_adj;
    const double sy = (1.0 - (((double)y + 0.5) / (double)h) * 2.0) * fov_adj;
    const double vx = sx, vy = sy, vz = -1.0;
    const double inv = 1.0 / std::sqrt((vx * vx + vy * vy) + vz * vz);
    o[0] = o[1] = o[2] = 0.0;
    d[0] = vx * inv;
    d[1] = vy * inv;
    d[2] = vz * inv;
}

static void camera_ray(const double eye[3], const double r[3], const double u[3], const double f[3], uint32_t x,
                       uint32_t y, uint32_t w, uint32_t h, double fov_adj, double o[3], double d[3]) {
    double sx, sy;
    rg_camera_sensor(x, y, (double)w, (double)h, (double)w / (double)h, fov_adj, &sx, &sy);
    CHECK(bits(sx) != bits(-0.0) && bits(sy) != bits(-0.0));  // never -0 (rg_camera.h)
    rg_camera_direction(r, u, f, sx, sy, d);
    for (int k = 0; k < 3; ++k) o[k] = eye[k];
}

static void identity_rays() {
    const uint32_t sizes[4][2] = {{1, 1}, {17, 3}, {97, 61}, {64, 48}};
    const double fovs[3] = {std::tan(90.0 * (3.14159265358979323846 / 180.0) / 2.0),
                            std::tan(60.0 * (3.14159265358979323846 / 180.0) / 2.0),
                            std::tan(120.0 * (3.14159265358979323846 / 180.0) / 2.0)};
    double lr[3], lu[3], lf[3];
    const double target[3] = {0.0, 0.0, -1.0};
    CHECK(rg_camera_look_at_basis(kEye0, target, kUp, lr, lu, lf));
    for (const auto &s : sizes)
        for (double fov : fovs) {
            unsigned long long bad = 0, bad_look = 0;
            for (uint32_t y = 0; y < s[1]; ++y)
                for (uint32_t x = 0; x < s[0]; ++x) {
                    double o0[3], d0[3], o1[3], d1[3], o2[3], d2[3];
                    create_prime(x, y, s[0], s[1], fov, o0, d0);
                    camera_ray(kEye0, kRight, kUp, kFwd, x, y, s[0], s[1], fov, o1, d1);
                    camera_ray(kEye0, lr, lu, lf, x, y, s[0], s[1], fov, o2, d2);
                    for (int k = 0; k < 3; ++k) {
                        if (bits(o0[k]) != bits(o1[k]) || bits(d0[k]) != bits(d1[k])) ++bad;
                        if (bits(o1[k]) != bits(o2[k]) || bits(d1[k]) != bits(d2[k])) ++bad_look;
                    }
                }
            if (bad || bad_look) std::printf("%ux%u fov %.17g: %llu / %llu components differ\n", s[0], s[1], fov, bad, bad_look);
            CHECK(bad == 0);
            CHECK(bad_look == 0);
        }
}

static double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

static void orthonormal() {
    const double poses[6][9] = {
        {3, 2, -10, 0, 0, -30, 0, 1, 0},        {0, 25, -40, 0, 0, -40, 0, 0, -1},  // straight down, up = -z
        {-7.5, 1.25, 4, 2, 0.5, -60, 0, 1, 0},  {1e6, 2e6, -3e6, 0, 0, -30, 0, 1, 0},
        {0, 0, 0, 1, 1, 1, 0.3, 1, -0.2},       {12, -3, -55, -12, 9, -20, 1, 0, 0},
    };
    const double tol = 4.0 * std::numeric_limits<double>::epsilon();  // 4 ulp of 1.0
    for (const auto &p : poses) {
        double r[3], u[3], f[3];
        CHECK(rg_camera_look_at_basis(p, p + 3, p + 6, r, u, f));
        const double e[6] = {dot3(r, r) - 1.0, dot3(u, u) - 1.0, dot3(f, f) - 1.0, dot3(r, u), dot3(r, f), dot3(u, f)};
        for (double v : e) {
            if (!(std::fabs(v) <= tol)) std::printf("pose eye (%g,%g,%g): residual %.3g\n", p[0], p[1], p[2], v);
            CHECK(std::fabs(v) <= tol);
        }
        // f points from the eye at the target, u to the up hint's side
        const double t[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]};
        CHECK(dot3(f, t) > 0.0);
        CHECK(dot3(u, p + 6) > 0.0);
    }
}

static void rejected() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double e[3] = {1, 2, 3}, t[3] = {1, 2, -3}, up[3] = {0, 1, 0};
    double r[3] = {7, 7, 7}, u[3] = {7, 7, 7}, f[3] = {7, 7, 7};
    auto untouched = [&] { return r[0] == 7 && u[1] == 7 && f[2] == 7; };
    CHECK(!rg_camera_look_at_basis(e, e, up, r, u, f));  // target == eye
    const double par[3] = {0, 0, 2}, anti[3] = {0, 0, -5}, zero[3] = {0, 0, 0};
    CHECK(!rg_camera_look_at_basis(e, t, par, r, u, f));   // up hint parallel to the view direction
    CHECK(!rg_camera_look_at_basis(e, t, anti, r, u, f));  // ... and anti-parallel
    CHECK(!rg_camera_look_at_basis(e, t, zero, r, u, f));  // ... and zero
    for (int k = 0; k < 3; ++k)
        for (double bad : {inf, -inf, nan}) {
            double b[3] = {1, 2, 3};
            b[k] = bad;
            CHECK(!rg_camera_look_at_basis(b, t, up, r, u, f));
            CHECK(!rg_camera_look_at_basis(e, b, up, r, u, f));
            CHECK(!rg_camera_look_at_basis(e, t, b, r, u, f));
            CHECK(!rg_camera_valid(b, kRight, kUp, kFwd));
            CHECK(!rg_camera_valid(kEye0, b, kUp, kFwd));
            CHECK(!rg_camera_valid(kEye0, kRight, b, kFwd));
            CHECK(!rg_camera_valid(kEye0, kRight, kUp, b));
        }
    CHECK(untouched());
    CHECK(!rg_camera_valid(kEye0, kRight, kUp, zero));  // forward all zero
    const double negzero[3] = {-0.0, 0.0, -0.0};
    CHECK(!rg_camera_valid(kEye0, kRight, kUp, negzero));
    CHECK(rg_camera_valid(kEye0, zero, zero, kFwd));  // a degenerate sensor is still a camera
    CHECK(rg_camera_valid(kEye0, kRight, kUp, kFwd));
}

int main(int argc, char **argv) {
    if (argc == 11 && !std::strcmp(argv[1], "look_at")) {
        double v[9], r[3], u[3], f[3];
        for (int k = 0; k < 9; ++k) v[k] = std::strtod(argv[2 + k], nullptr);
        if (!rg_camera_look_at_basis(v, v + 3, v + 6, r, u, f)) {
            std::puts("rejected");
            return 0;
        }
        std::printf("%a %a %a %a %a %a %a %a %a\n", r[0], r[1], r[2], u[0], u[1], u[2], f[0], f[1], f[2]);
        return 0;
    }
    identity_rays();
    orthonormal();
    rejected();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::puts("ok");
    return 0;
}
