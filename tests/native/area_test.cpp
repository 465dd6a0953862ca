// area_test.cpp — raingun_amd/csrc/rg_area.h on the CPU (tests/test_area_cpu.py builds and runs it, once more
// with AddressSanitizer + UBSan as its own executable).
//   area_test            the checks below, then "ok"
//   area_test eval       reads lines "k W x y l r vx vy vz" from stdin and prints, per line, "j m px py pz" of
//                        rg_area_index / rg_area_position (the doubles as %a) with the header's own host tables:
//                        tests/test_area_cpu.py compares them with its numpy statement of the rule
// The checks:
//   * the key and a hand-computed index: pixel (0, 0), light 0 hashes lowbias32(0x9e3779b9)
//   * the table layout: 3 doubles per point, k's points behind 1 + 4 + .. + (k - 1)^2 others, the radii behind 204
//   * the host points: |p| = 1 within 4 ulp, mean 0 within 1e-15 for k >= 2, z of row-major cell (i, j) is 1 - 2u
//   * radius 0 gives the centre's bits; a radius moves the light by exactly that distance (within rounding)
//   * the k^2 samples of an output pixel take k^2 distinct points (the shift is a permutation)
//   * rg_area_active, rg_area_radius_valid
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../raingun_amd/csrc/rg_area.h"

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

static std::vector<double> g_points(RG_AREA_POINT_DOUBLES), g_rot(2 * RG_LENS_ROTATIONS);

static void index_rule() {
    CHECK(RG_AREA_KEY == 0x9e3779b9u);
    uint32_t j, m;
    // pixel (0, 0) of any frame, light 0: s = 0, n = 0, g = lowbias32(key)
    const uint32_t g = rg_lens_hash(0x9e3779b9u);
    rg_area_index(0, 0, 4, 96, 0, &j, &m);
    CHECK(j == (g >> 6) % 16u && m == (g & 63u));
    // the sample adds to the shift: pixel (1, 2) of the same output pixel is sample 2 * 4 + 1
    uint32_t j2, m2;
    rg_area_index(1, 2, 4, 96, 0, &j2, &m2);
    CHECK(j2 == (9u + (g >> 6)) % 16u && m2 == m);
    // the next output pixel and the next light hash other words: n = 1, l = 1 (the product wraps)
    rg_area_index(4, 0, 4, 96, 0, &j2, &m2);
    CHECK(m2 == (rg_lens_hash(1u ^ 0x9e3779b9u) & 63u));
    rg_area_index(0, 0, 4, 96, 1, &j2, &m2);
    CHECK(m2 == (rg_lens_hash((uint32_t)(2ull * 0x9e3779b9ull)) & 63u));
    // the row of the output pixel counts W, not kW
    rg_area_index(0, 4, 4, 96, 0, &j2, &m2);
    CHECK(m2 == (rg_lens_hash(96u ^ 0x9e3779b9u) & 63u));
    // k = 1: one point, whatever the hash
    rg_area_index(17, 5, 1, 40, 2, &j2, &m2);
    CHECK(j2 == 0u);
    // the k^2 samples of a pixel: a permutation of the k^2 points, for every light
    for (uint32_t k = 1; k <= RG_LENS_MAX_SAMPLES; ++k)
        for (uint32_t l = 0; l < 3; ++l) {
            bool seen[64] = {};
            uint32_t turn = 64;
            for (uint32_t y = 0; y < k; ++y)
                for (uint32_t x = 0; x < k; ++x) {
                    rg_area_index(5 * k + x, 3 * k + y, k, 40, l, &j, &m);
                    CHECK(j < k * k && !seen[j]);
                    seen[j] = true;
                    CHECK(turn == 64 || turn == m);  // one turn per output pixel and light
                    turn = m;
                }
        }
}

static void layout_and_points() {
    CHECK(RG_AREA_POINT_DOUBLES == 3 * 204 && rg_area_table_doubles(0) == 612u && rg_area_table_doubles(5) == 617u);
    const double eps = std::numeric_limits<double>::epsilon();
    for (uint32_t k = 1; k <= RG_LENS_MAX_SAMPLES; ++k) {
        const double *p = g_points.data() + 3u * rg_lens_points_offset(k);
        std::vector<double> own(3u * k * k);
        rg_area_make_points(k, own.data());
        CHECK(std::memcmp(own.data(), p, own.size() * sizeof(double)) == 0);  // the table holds k's points at its offset
        double mean[3] = {0.0, 0.0, 0.0};
        for (uint32_t c = 0; c < k * k; ++c) {
            const double n2 = (p[3 * c] * p[3 * c] + p[3 * c + 1] * p[3 * c + 1]) + p[3 * c + 2] * p[3 * c + 2];
            CHECK(std::fabs(std::sqrt(n2) - 1.0) <= 4.0 * eps);
            for (int a = 0; a < 3; ++a) mean[a] += p[3 * c + a] / (double)(k * k);
            CHECK(bits(p[3 * c + 2]) == bits(1.0 - 2.0 * (((double)(c % k) + 0.5) / (double)k)));  // cell (i, j) at j * k + i
        }
        if (k >= 2)
            for (int a = 0; a < 3; ++a) CHECK(std::fabs(mean[a]) <= 1e-15);
    }
    // k = 1: the one point is on the equator at phi = pi: (-1, ~0, 0)
    CHECK(g_points[0] == -1.0 && std::fabs(g_points[1]) <= 2e-16 && g_points[2] == 0.0);
}

static void positions() {
    const double v[3] = {1.5, 5.0, -4.0};
    for (uint32_t k = 1; k <= RG_LENS_MAX_SAMPLES; ++k) {
        const double *pk = g_points.data() + 3u * rg_lens_points_offset(k);
        for (uint32_t y = 0; y < 2 * k; ++y)
            for (uint32_t x = 0; x < 3 * k; ++x) {
                double pos[3];
                rg_area_position(v, 0.0, x, y, k, 3, 1, pk, g_rot.data(), pos);
                CHECK(bits(pos[0]) == bits(v[0]) && bits(pos[1]) == bits(v[1]) && bits(pos[2]) == bits(v[2]));
                rg_area_position(v, 1.5, x, y, k, 3, 1, pk, g_rot.data(), pos);
                const double d = std::sqrt(((pos[0] - v[0]) * (pos[0] - v[0]) + (pos[1] - v[1]) * (pos[1] - v[1])) +
                                           (pos[2] - v[2]) * (pos[2] - v[2]));
                CHECK(std::fabs(d - 1.5) <= 1e-14);
            }
    }
}

static void predicates() {
    CHECK(!rg_area_active(false, 4) && !rg_area_active(true, 1) && !rg_area_active(true, 0) && rg_area_active(true, 2) &&
          rg_area_active(true, 8));
    CHECK(rg_area_radius_valid(0.0) && rg_area_radius_valid(1e300) && !rg_area_radius_valid(-1e-300) &&
          !rg_area_radius_valid(std::numeric_limits<double>::infinity()) &&
          !rg_area_radius_valid(std::numeric_limits<double>::quiet_NaN()));
}

static int eval_stdin() {
    unsigned k, w, x, y, l;
    double r, v[3];
    while (std::scanf("%u %u %u %u %u %lf %lf %lf %lf", &k, &w, &x, &y, &l, &r, &v[0], &v[1], &v[2]) == 9) {
        if (k < 1 || k > RG_LENS_MAX_SAMPLES) return 2;
        uint32_t j, m;
        double pos[3];
        rg_area_index(x, y, k, w, l, &j, &m);
        rg_area_position(v, r, x, y, k, w, l, g_points.data() + 3u * rg_lens_points_offset(k), g_rot.data(), pos);
        std::printf("%u %u %a %a %a\n", j, m, pos[0], pos[1], pos[2]);
    }
    return 0;
}

int main(int argc, char **argv) {
    rg_area_make_table_points(g_points.data());
    rg_lens_make_rotations(g_rot.data());
    if (argc > 1 && !std::strcmp(argv[1], "eval")) return eval_stdin();
    index_rule();
    layout_and_points();
    positions();
    predicates();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::puts("ok");
    return 0;
}
