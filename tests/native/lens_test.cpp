// lens_test.cpp — raingun_amd/csrc/rg_lens.h on the CPU (tests/test_lens_cpu.py builds and runs it).
//   * the hash (lowbias32) on fixed values, against constants and an independent 64-bit evaluation of its five steps
//   * the table offsets: k's points start behind 1 + 4 + .. + (k - 1)^2 others, 204 in all
//   * the lens ray of hand-computed samples: identity camera, aperture 2, focus 4, k = 2, chosen so that
//     every intermediate is a small dyadic number and the expected origin and V are exact
//   * a point table of zeros and focus 1 give the camera ray of rg_camera_direction bit for bit
//   * aperture == 0 and samples == 1 are reported as "no lens"; bad lenses are no lenses
//   * the host tables: (0, 0) for k = 1 and the centre cell of odd k, every point inside the unit disk
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../raingun_amd/csrc/rg_lens.h"

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

static void hash_values() {
    // 0 stays 0 through every step; the others against an independent 64-bit evaluation of the five steps
    CHECK(rg_lens_hash(0u) == 0u);
    auto slow = [](uint32_t n) {
        uint64_t v = n;
        v ^= v >> 16;
        v = (v * 0x7feb352dull) & 0xffffffffull;
        v ^= v >> 15;
        v = (v * 0x846ca68bull) & 0xffffffffull;
        v ^= v >> 16;
        return (uint32_t)v;
    };
    const uint32_t fixed[6] = {1u, 2u, 63u, 64u, 0x12345678u, 0xffffffffu};
    const uint32_t want[6] = {0x688990c0u, 0xd1132181u, 0xd3a3cc1eu, 0xdce420bau, 0xf5e71c96u, 0x6768824au};
    for (int i = 0; i < 6; ++i) CHECK(rg_lens_hash(fixed[i]) == want[i] && slow(fixed[i]) == want[i]);
    // the first step by hand: 1 -> 0x7feb352d, whose top half is 0x7feb, >> 15 is 0xffd6
    CHECK((0x7feb352du >> 15) == 0xffd6u);
    CHECK(rg_lens_hash(1u) == (uint32_t)((((0x7feb352dull ^ 0xffd6ull) * 0x846ca68bull) & 0xffffffffull) ^
                                         ((((0x7feb352dull ^ 0xffd6ull) * 0x846ca68bull) & 0xffffffffull) >> 16)));
    // it spreads consecutive pixels over the 64 turns: the first 256 indices hit at least 48 of them
    bool seen[64] = {};
    int distinct = 0;
    for (uint32_t n = 0; n < 256u; ++n)
        if (!seen[rg_lens_hash(n) & 63u]) { seen[rg_lens_hash(n) & 63u] = true; ++distinct; }
    CHECK(distinct >= 48);
}

static void offsets() {
    uint32_t sum = 0;
    for (uint32_t k = 1; k <= RG_LENS_MAX_SAMPLES; ++k) {
        CHECK(rg_lens_points_offset(k) == sum);
        sum += k * k;
    }
    CHECK(sum == RG_LENS_POINTS);
    CHECK(RG_LENS_TABLE_DOUBLES == 2 * 204 + 128);
}

// rotations with one entry everywhere: every pixel gets the same turn, whatever its hash
static void fill_rotations(double *rot, double c, double g) {
    for (int m = 0; m < RG_LENS_ROTATIONS; ++m) { rot[2 * m] = c; rot[2 * m + 1] = g; }
}

static void hand_computed_rays() {
    // identity camera, k = 2, a 4 x 2 output frame (sample frame 8 x 4), aperture 2, focus 4
    // LR = (2, 0, 0), LU = (0, 2, 0).  Points: s = 0 (0.5, 0), s = 1 (0, 0.5), s = 2 (-0.25, 0.25), s = 3 (0, 0).
    const double points[8] = {0.5, 0.0, 0.0, 0.5, -0.25, 0.25, 0.0, 0.0};
    double rot[128], lr[3], lu[3];
    rg_lens_axis(kRight, 2.0, lr);
    rg_lens_axis(kUp, 2.0, lu);
    CHECK(lr[0] == 2.0 && lr[1] == 0.0 && lr[2] == 0.0 && lu[0] == 0.0 && lu[1] == 2.0 && lu[2] == 0.0);
    const double sx = 0.75, sy = -0.5;  // D = (0.75, -0.5, -1), D * 4 = (3, -2, -4)
    struct Case { uint32_t x, y; double c, g, ox, oy, vx, vy; };
    const Case cases[5] = {
        // no turn (c 1, g 0): q = p.  s 0: O = (1, 0);  V = (3 - 1, -2 - 0, -4)
        {4, 2, 1.0, 0.0, 1.0, 0.0, 2.0, -2.0},
        // s 1 (x odd, y even): O = (0, 1); V = (3, -3, -4)
        {5, 2, 1.0, 0.0, 0.0, 1.0, 3.0, -3.0},
        // s 2 (x even, y odd): O = (-0.5, 0.5); V = (3.5, -2.5, -4)
        {4, 3, 1.0, 0.0, -0.5, 0.5, 3.5, -2.5},
        // a quarter turn (c 0, g 1): q = (-pv, pu).  s 0: q = (0, 0.5), O = (0, 1)
        {0, 0, 0.0, 1.0, 0.0, 1.0, 3.0, -3.0},
        // s 2 under the quarter turn: q = (-0.25, -0.25), O = (-0.5, -0.5); V = (3.5, -1.5, -4)
        {6, 1, 0.0, 1.0, -0.5, -0.5, 3.5, -1.5},
    };
    for (const Case &t : cases) {
        fill_rotations(rot, t.c, t.g);
        double o[3], d[3];
        rg_lens_ray(kEye0, kRight, kUp, kFwd, sx, sy, t.x, t.y, 2u, 4u, 4.0, lr, lu, points, rot, o, d);
        const double v[3] = {t.vx, t.vy, -4.0};
        double want[3];
        rg_camera_normalize(v, want);
        CHECK(o[0] == t.ox && o[1] == t.oy && o[2] == 0.0);
        for (int i = 0; i < 3; ++i) CHECK(bits(d[i]) == bits(want[i]));
        // the ray meets the plane in focus (z = -4) where the pinhole ray does: at D * focus
        const double s = -4.0 / d[2];
        CHECK(std::fabs(o[0] + s * d[0] - 3.0) < 1e-14 && std::fabs(o[1] + s * d[1] + 2.0) < 1e-14);
    }
    // the centre sample (s 3, the point (0, 0)) leaves the eye, an eye that is not the origin included
    const double eye[3] = {1.5, -2.0, 8.0};
    fill_rotations(rot, 0.6, 0.8);
    double o[3], d[3], want[3];
    rg_lens_ray(eye, kRight, kUp, kFwd, sx, sy, 7u, 3u, 2u, 4u, 4.0, lr, lu, points, rot, o, d);
    const double v[3] = {3.0, -2.0, -4.0};
    rg_camera_normalize(v, want);
    CHECK(o[0] == 1.5 && o[1] == -2.0 && o[2] == 8.0);
    for (int i = 0; i < 3; ++i) CHECK(bits(d[i]) == bits(want[i]));
    // the turn is the output pixel's: the four samples of a pixel share it, the next pixel may differ
    for (int m = 0; m < RG_LENS_ROTATIONS; ++m) { rot[2 * m] = (double)m; rot[2 * m + 1] = 0.0; }
    const double unit[8] = {1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0};
    for (uint32_t py = 0; py < 2u; ++py)
        for (uint32_t px = 0; px < 4u; ++px) {
            const double turn = (double)(rg_lens_hash(py * 4u + px) & 63u);
            for (uint32_t j = 0; j < 2u; ++j)
                for (uint32_t i = 0; i < 2u; ++i) {
                    rg_lens_ray(kEye0, kRight, kUp, kFwd, sx, sy, 2u * px + i, 2u * py + j, 2u, 4u, 4.0, lr, lu, unit, rot, o, d);
                    CHECK(o[0] == 2.0 * turn && o[1] == 0.0);  // O = LR * (c * 1) with c = m
                }
        }
}

static void zero_points_are_the_camera() {
    const double zeros[2 * 9] = {};
    double rot[128];
    rg_lens_make_rotations(rot);
    const double eye[3] = {3.0, 2.0, -10.0}, r[3] = {0.8, 0.0, 0.6}, u[3] = {0.1, 1.0, -0.2}, f[3] = {0.6, -0.1, -0.8};
    double lr[3], lu[3];
    rg_lens_axis(r, 0.75, lr);
    rg_lens_axis(u, 0.75, lu);
    for (uint32_t y = 0; y < 9u; ++y)
        for (uint32_t x = 0; x < 12u; ++x) {
            double sx, sy, o[3], d[3], want[3];
            rg_camera_sensor(x, y, 12.0, 9.0, 12.0 / 9.0, 1.0, &sx, &sy);
            rg_lens_ray(eye, r, u, f, sx, sy, x, y, 3u, 4u, 1.0, lr, lu, zeros, rot, o, d);
            rg_camera_direction(r, u, f, sx, sy, want);
            for (int i = 0; i < 3; ++i) CHECK(o[i] == eye[i] && bits(d[i]) == bits(want[i]));
        }
}

static void no_lens() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(!rg_lens_active(0.0, 4u));   // aperture == 0: a pinhole
    CHECK(!rg_lens_active(0.5, 1u));   // one sample per pixel
    CHECK(!rg_lens_active(0.0, 1u));
    CHECK(!rg_lens_active(-0.0, 2u));
    CHECK(rg_lens_active(0.5, 2u) && rg_lens_active(1e-300, 8u));
    CHECK(rg_lens_valid(0.0, 1.0) && rg_lens_valid(2.5, 1e-3));
    CHECK(!rg_lens_valid(-1.0, 1.0) && !rg_lens_valid(1.0, 0.0) && !rg_lens_valid(1.0, -2.0));
    for (double bad : {inf, -inf, nan}) CHECK(!rg_lens_valid(bad, 1.0) && !rg_lens_valid(1.0, bad));
}

static void host_tables() {
    double table[RG_LENS_TABLE_DOUBLES];
    rg_lens_make_tables(table);
    CHECK(bits(table[0]) == bits(0.0) && bits(table[1]) == bits(0.0));  // k = 1
    for (uint32_t k = 1; k <= RG_LENS_MAX_SAMPLES; ++k) {
        const double *p = table + 2 * rg_lens_points_offset(k);
        for (uint32_t s = 0; s < k * k; ++s) CHECK(p[2 * s] * p[2 * s] + p[2 * s + 1] * p[2 * s + 1] <= 1.0);
        if (k % 2u == 1u) {
            const uint32_t c = (k / 2u) * k + k / 2u;
            CHECK(bits(p[2 * c]) == bits(0.0) && bits(p[2 * c + 1]) == bits(0.0));
        }
    }
    const double *rot = table + 2 * RG_LENS_POINTS;
    CHECK(rot[0] == 1.0 && rot[1] == 0.0);
    for (int m = 0; m < RG_LENS_ROTATIONS; ++m)
        CHECK(std::fabs(rot[2 * m] * rot[2 * m] + rot[2 * m + 1] * rot[2 * m + 1] - 1.0) <= 1e-15);
}

int main() {
    hash_values();
    offsets();
    hand_computed_rays();
    zero_points_are_the_camera();
    no_lens();
    host_tables();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::puts("ok");
    return 0;
}
