// The exact replacements of raingun_amd/csrc/rg_exact.h against the operations they replace, on the
// CPU: a stand-alone program over the header alone (tests/test_exact_div.py compiles it with
// g++ -O2 -ffp-contract=off; C fma, no contraction).  Prints one line per check and "ok" at the end.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raingun_amd/csrc/rg_exact.h"

static int failures = 0;
#define CHECK(cond)                                               \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            ++failures;                                           \
        }                                                         \
    } while (0)

static uint64_t bits(double v) {
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}
static double from_bits(uint64_t b) {
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}

// ---- the camera quotients: (i + 0.5) / n for every n <= 20000 and every i < n
static void quotients() {
    unsigned long long pairs = 0, bad = 0, bad_q0 = 0;
    for (uint32_t n = 1; n <= 20000; ++n) {
        const double nd = (double)n, inv = 1.0 / nd;
        for (uint32_t i = 0; i < n; ++i) {
            const double a = (double)i + 0.5, q = a / nd;
            bad += bits(rg_recip_quot(a, nd, inv)) != bits(q);
            bad_q0 += bits(a * inv) != bits(q);
            ++pairs;
        }
    }
    std::printf("quotient: %llu pairs, %llu mismatches (the bare product a * inv: %llu)\n", pairs, bad, bad_q0);
    CHECK(pairs == 200010000ull);
    CHECK(bad == 0);
    CHECK(bad_q0 > 0);  // the residual step is what makes it exact
    unsigned ok = 0, up = 0, down = 0;
    for (uint32_t n = 1; n <= 20000; ++n) {
        const double inv = 1.0 / (double)n;
        ok += rg_recip_div_ok(n);
        up += rg_recip_div_ok(n, from_bits(bits(inv) + 1));
        down += rg_recip_div_ok(n, from_bits(bits(inv) - 1));
    }
    std::printf("rg_recip_div_ok: %u of 20000 sizes admitted; reciprocal an ulp up: %u, an ulp down: %u\n", ok, up, down);
    CHECK(ok == 20000);
    CHECK(up == 0 && down == 0);
    CHECK(!rg_recip_div_ok(0));
}

// ---- the modulo of material.rs:70-79 and the unsigned division under it
static uint32_t wrap_ref(int32_t w, int32_t max) {  // the kernel's wrap() after the cast (rg_k_shade.h)
    int32_t r = w % max;
    return r < 0 ? (uint32_t)(r + max) : (uint32_t)r;
}
static void modulo() {
    std::vector<uint32_t> divisors;
    for (uint32_t d = 1; d <= 4096; ++d) divisors.push_back(d);
    for (int k = 0; k <= 30; ++k) {
        const uint32_t p = 1u << k;
        divisors.push_back(p);
        divisors.push_back(p + 1);
        if (p > 1) divisors.push_back(p - 1);
    }
    divisors.push_back(2147483647u);
    for (uint32_t d : {1500u, 2048u, 1024u, 512u}) divisors.push_back(d);  // the golden textures' sides
    std::vector<int32_t> random;
    uint64_t s = 0x9E3779B97F4A7C15ull;  // splitmix64, fixed seed
    for (int i = 0; i < 100000; ++i) {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        random.push_back((int32_t)(uint32_t)((z ^ (z >> 31)) >> 16));
    }
    unsigned long long cases = 0, bad = 0, bad_div = 0;
    for (uint32_t d : divisors) {
        const RgMagicU32 g = rg_magic_u32(d);
        std::vector<int64_t> w = {INT_MIN, INT_MIN + 1ll, INT_MAX};
        // every value within 1 of a multiple of d near 0 and near +-2^31
        const int64_t dd = (int64_t)d, top = (int64_t)(2147483648ll / dd) * dd;
        const int64_t bases[] = {0, dd, -dd, 2 * dd, -2 * dd, top, top - dd, -top, -top + dd};
        for (int64_t base : bases)
            for (int64_t e = -1; e <= 1; ++e) w.push_back(base + e);
        auto one = [&](int32_t x) {
            bad += rg_wrap_i32(x, d, g.m, g.sh) != wrap_ref(x, (int32_t)d);
            const uint32_t u = (uint32_t)x;  // the same bits as an unsigned dividend (tile indices, rows)
            bad_div += rg_magic_div(u, g.m, g.sh) != u / d;
            ++cases;
        };
        for (int64_t v : w)
            if (v >= INT_MIN && v <= INT_MAX) one((int32_t)v);
        for (int32_t r : random) one(r);
        bad_div += rg_magic_div(0xFFFFFFFFu, g.m, g.sh) != 0xFFFFFFFFu / d;
    }
    std::printf("modulo: %zu divisors, %llu cases, %llu mismatches; unsigned quotient: %llu mismatches\n", divisors.size(),
                cases, bad, bad_div);
    CHECK(bad == 0);
    CHECK(bad_div == 0);
    // divisors above 2^31 (tile counts never get there; the magic still holds)
    for (uint32_t d : {0x80000001u, 0xFFFFFFFFu, 0xC0000000u}) {
        const RgMagicU32 g = rg_magic_u32(d);
        for (uint32_t n : {0u, 1u, d - 1, d, d + 1, 0xFFFFFFFFu}) CHECK(rg_magic_div(n, g.m, g.sh) == n / d);
    }
}

// ---- the planes' texture axes: texture_coords' expressions (rg_k_shade.h, rg_k_math.h), restated
struct V3 {
    double x, y, z;
};
static V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static void axes() {
    const double normals[][3] = {{0, -1, 0}, {0, 0, 1},        {0, 0, -1},          {0, 1, 0},
                                 {0.6, 0, 0.8}, {-0.3, 0.5, 0.2}, {0.1, -7.25, 3.0}, {-0.0, 0.0, 2.0}};
    unsigned fallback = 0;
    for (const auto &nn : normals) {
        const V3 n{nn[0], nn[1], nn[2]};
        V3 xa = cross(n, V3{0.0, 0.0, 1.0});
        if (dot(xa, xa) == 0.0) {
            xa = cross(n, V3{0.0, 1.0, 0.0});
            ++fallback;
        }
        const V3 ya = cross(n, xa);
        double hx[3], hy[3];
        rg_plane_axes(nn, hx, hy);
        CHECK(bits(hx[0]) == bits(xa.x) && bits(hx[1]) == bits(xa.y) && bits(hx[2]) == bits(xa.z));
        CHECK(bits(hy[0]) == bits(ya.x) && bits(hy[1]) == bits(ya.y) && bits(hy[2]) == bits(ya.z));
    }
    std::printf("axes: %zu normals, %u on the fallback axis\n", sizeof normals / sizeof normals[0], fallback);
    CHECK(fallback == 3);  // the normals along z
}

// ---- the camera ray's range predicate
static void camera_range() {
    CHECK(rg_camera_unscaled_ok(0.0, 1.0));
    CHECK(rg_camera_unscaled_ok(1.0, 16.0 / 9.0));
    CHECK(rg_camera_unscaled_ok(114.58865012930961, 512.0));  // fov 179 degrees, 4096 x 8
    CHECK(rg_camera_unscaled_ok(-1.0, 2.0));                  // a reflex field of view: the square decides
    CHECK(rg_camera_unscaled_ok(5e14, 1.0));                  // s = 5e29, below 2^100 = 1.27e30
    CHECK(!rg_camera_unscaled_ok(1e15, 1.0));                 // s = 2e30
    CHECK(!rg_camera_unscaled_ok(1e16, 1.0));
    CHECK(!rg_camera_unscaled_ok(1.0, 1e16));
    CHECK(!rg_camera_unscaled_ok(1e200, 1e200));              // overflows to inf
    const double nan = from_bits(0x7ff8000000000000ull);
    CHECK(!rg_camera_unscaled_ok(nan, 1.0));
    CHECK(!rg_camera_unscaled_ok(1.0, nan));
}

int main(int argc, char **argv) {
    const bool all = argc < 2;
    if (all || !std::strcmp(argv[1], "quotients")) quotients();
    if (all || !std::strcmp(argv[1], "modulo")) modulo();
    if (all || !std::strcmp(argv[1], "axes")) axes();
    if (all || !std::strcmp(argv[1], "camera")) camera_range();
    std::printf(failures ? "failed\n" : "ok\n");
    return failures ? 1 : 0;
}
