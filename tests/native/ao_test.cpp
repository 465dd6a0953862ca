// ao_test.cpp — raingun_amd/csrc/rg_ao.h on the CPU (tests/test_ao_cpu.py builds and runs it, once more with
// AddressSanitizer + UBSan as its own executable).  Prints "ok" after the checks:
//   * the table layout: 3 doubles per point, k's points behind 1 + 4 + .. + (k - 1)^2 others, the 64 turns behind 204
//   * the host points: unit length within 4 ulp, z >= 0, k = 1 and the centre cell of odd k exactly (0, 0, 1),
//     (x, y) the lens's points
//   * the facing normal: unit, on the ray's side, sign kept for dot == 0
//   * the tangent frame: (T, B, nf) orthonormal within rounding for normals that include (0,0,+-1), (0,0,-0.0),
//     the axes and a few hundred others; right-handed (T x B = nf)
//   * the turned frame: orthonormal again, the turn 0 the frame's bits, the turn's angle about nf
//   * a sample's direction: unit, in the facing hemisphere, (0,0,1) -> nf
//   * rg_ao_valid
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../raingun_amd/csrc/rg_ao.h"

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
static double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

static const double EPS = std::numeric_limits<double>::epsilon();
static std::vector<double> g_table(RG_AO_TABLE_DOUBLES);

static void tables() {
    CHECK(RG_AO_POINT_DOUBLES == 3 * 204 && RG_AO_TABLE_DOUBLES == 3 * 204 + 128 && RG_AO_MAX_SAMPLES == 8);
    rg_ao_make_table(g_table.data());
    double rot[2 * RG_LENS_ROTATIONS];
    rg_lens_make_rotations(rot);
    CHECK(std::memcmp(rot, g_table.data() + RG_AO_POINT_DOUBLES, sizeof rot) == 0);
    for (uint32_t k = 1; k <= 8; ++k) {
        std::vector<double> p(3 * k * k), disk(2 * k * k);
        rg_ao_make_points(k, p.data());
        rg_lens_make_points(k, disk.data());
        CHECK(std::memcmp(p.data(), g_table.data() + 3 * rg_lens_points_offset(k), p.size() * sizeof(double)) == 0);
        for (uint32_t j = 0; j < k * k; ++j) {
            const double *q = &p[3 * j];
            CHECK(bits(q[0]) == bits(disk[2 * j]) && bits(q[1]) == bits(disk[2 * j + 1]));
            CHECK(q[2] >= 0.0 && std::fabs(dot3(q, q) - 1.0) <= 4 * EPS);
        }
        if (k % 2 == 1) {
            const double *c = &p[3 * ((k / 2) * k + k / 2)];
            CHECK(c[0] == 0.0 && c[1] == 0.0 && c[2] == 1.0);
        }
    }
}

static void check_frame(const double nf[3]) {
    double t[3], b[3];
    rg_ao_frame(nf, t, b);
    const double tol = 8 * EPS;
    CHECK(std::fabs(dot3(t, t) - 1.0) <= tol && std::fabs(dot3(b, b) - 1.0) <= tol);
    CHECK(std::fabs(dot3(t, b)) <= tol && std::fabs(dot3(t, nf)) <= tol && std::fabs(dot3(b, nf)) <= tol);
    double c[3];
    rg_camera_cross(t, b, c);
    CHECK(std::fabs(c[0] - nf[0]) <= tol && std::fabs(c[1] - nf[1]) <= tol && std::fabs(c[2] - nf[2]) <= tol);
    // the turned frame: turn 0 keeps the bits (1 * v + 0 * w), every turn keeps the frame orthonormal
    const double *rot = g_table.data() + RG_AO_POINT_DOUBLES;
    double tr[3], br[3];
    rg_ao_turn(t, b, rot[0], rot[1], tr, br);
    for (int i = 0; i < 3; ++i) CHECK(tr[i] == t[i] && br[i] == b[i]);
    for (uint32_t m = 0; m < 64; ++m) {
        rg_ao_turn(t, b, rot[2 * m], rot[2 * m + 1], tr, br);
        CHECK(std::fabs(dot3(tr, tr) - 1.0) <= tol && std::fabs(dot3(br, br) - 1.0) <= tol);
        CHECK(std::fabs(dot3(tr, br)) <= tol && std::fabs(dot3(tr, nf)) <= tol && std::fabs(dot3(br, nf)) <= tol);
        CHECK(std::fabs(dot3(tr, t) - rot[2 * m]) <= tol && std::fabs(dot3(tr, b) - rot[2 * m + 1]) <= tol);
        // every sample's direction: unit, not below the surface; the pole gives nf
        for (uint32_t k = 1; k <= 8; k += 7) {
            const double *p = g_table.data() + 3 * rg_lens_points_offset(k);
            for (uint32_t j = 0; j < k * k; ++j) {
                double d[3];
                rg_ao_direction(tr, br, nf, p[3 * j], p[3 * j + 1], p[3 * j + 2], d);
                CHECK(std::fabs(dot3(d, d) - 1.0) <= tol && dot3(d, nf) >= -tol);
                CHECK(std::fabs(dot3(d, nf) - p[3 * j + 2]) <= tol);
            }
        }
        double d[3];
        rg_ao_direction(tr, br, nf, 0.0, 0.0, 1.0, d);
        CHECK(std::fabs(d[0] - nf[0]) <= tol && std::fabs(d[1] - nf[1]) <= tol && std::fabs(d[2] - nf[2]) <= tol);
    }
}

static void frames() {
    const double special[][3] = {{0, 0, 1}, {0, 0, -1}, {0, 0, -0.0}, {1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0},
                                 {1, 0, -0.0}, {0, -1, -0.0}};
    for (const auto &s : special) {
        double nf[3];
        const double away[3] = {-s[0], -s[1], -s[2]};
        if (s[0] == 0 && s[1] == 0 && s[2] == 0) {  // (0, 0, -0.0) is no direction, but its frame is finite: s = -1
            double t[3], b[3];
            rg_ao_frame(s, t, b);
            CHECK(t[0] == 1.0 && t[1] == 0.0 && t[2] == 0.0 && b[0] == 0.0 && b[1] == -1.0 && b[2] == 0.0);
            continue;
        }
        rg_ao_facing(s, away, nf);
        CHECK(bits(nf[0]) == bits(s[0]) && bits(nf[1]) == bits(s[1]) && bits(nf[2]) == bits(s[2]));
        check_frame(nf);
    }
    {  // nf.z = -0.0 takes s = -1: a = -1 / (-1 + -0) = 1, finite, and the frame is still orthonormal
        const double nf[3] = {0.6, 0.8, -0.0};
        double t[3], b[3];
        rg_ao_frame(nf, t, b);
        CHECK(std::isfinite(t[0]) && std::isfinite(b[1]));
        check_frame(nf);
    }
    uint32_t seed = 12345u;
    for (int n = 0; n < 300; ++n) {
        double v[3];
        for (double &c : v) {
            seed = rg_lens_hash(seed + 0x9e3779b9u);
            c = (double)seed / 2147483648.0 - 1.0;
        }
        if (n % 7 == 0) v[2] = -std::fabs(v[2]) * 1e-9 - 1.0 * (n % 2);  // near and at the southern pole's side
        const double scale = n % 3 == 0 ? 17.5 : 1.0;                   // not unit: a plane's YAML normal
        const double raw[3] = {v[0] * scale, v[1] * scale, v[2] * scale};
        const double toward[3] = {-v[0], -v[1], -v[2]}, along[3] = {v[0], v[1], v[2]};
        double nf[3], nb[3];
        rg_ao_facing(raw, toward, nf);
        rg_ao_facing(raw, along, nb);
        CHECK(std::fabs(dot3(nf, nf) - 1.0) <= 4 * EPS && dot3(nf, toward) <= 0.0 && dot3(nb, along) <= 0.0);
        for (int i = 0; i < 3; ++i) CHECK(bits(nb[i]) == bits(-nf[i]));
        check_frame(nf);
        check_frame(nb);
        double o[3];
        const double h[3] = {1.0, -2.0, 3.0};
        rg_ao_origin(h, nf, 0.0, o);
        CHECK(o[0] == h[0] && o[1] == h[1] && o[2] == h[2]);
        rg_ao_origin(h, nf, 0.5, o);
        CHECK(o[0] == h[0] + nf[0] * 0.5 && o[2] == h[2] + nf[2] * 0.5);
    }
    {  // dot == 0 keeps m
        const double n[3] = {0, 2, 0}, d[3] = {1, 0, 0};
        double nf[3];
        rg_ao_facing(n, d, nf);
        CHECK(nf[0] == 0.0 && nf[1] == 1.0 && nf[2] == 0.0);
    }
    CHECK(rg_ao_turn_index(0u) == (rg_lens_hash(0u) & 63u) && rg_ao_turn_index(96u) == (rg_lens_hash(96u) & 63u));
}

static void validation() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(rg_ao_valid(1, inf, 1e-13) && rg_ao_valid(8, 0.5, 0.0) && rg_ao_valid(4, 1e-300, 1e-6));
    CHECK(!rg_ao_valid(0, 1.0, 0.0) && !rg_ao_valid(9, 1.0, 0.0) && !rg_ao_valid(0xFFFFFFFFu, 1.0, 0.0));
    CHECK(!rg_ao_valid(2, 0.0, 0.0) && !rg_ao_valid(2, -1.0, 0.0) && !rg_ao_valid(2, nan, 0.0) && !rg_ao_valid(2, -inf, 0.0));
    CHECK(!rg_ao_valid(2, 1.0, -1e-13) && !rg_ao_valid(2, 1.0, inf) && !rg_ao_valid(2, 1.0, nan));
    CHECK(rg_ao_valid(2, 1.0, -0.0));
}

int main() {
    tables();
    frames();
    validation();
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
