// The per-lane admission of the PLAIN kernels' unscaled sqrt / division (raingun_amd/csrc/rg_exact.h,
// DESIGN.md 4t), on the CPU: a stand-alone program over the header alone (tests/test_unscaled_cpu.py
// compiles it with g++ -O2 -ffp-contract=off).  Prints one line per check and "ok" at the end.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../raingun_amd/csrc/rg_exact.h"

static int failures = 0;
#define CHECK(cond)                                               \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            ++failures;                                           \
        }                                                         \
    } while (0)

static double from_bits(uint64_t b) {
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}
static double make(unsigned sign, unsigned biased, uint64_t mantissa) {
    return from_bits(((uint64_t)sign << 63) | ((uint64_t)biased << 52) | (mantissa & 0xFFFFFFFFFFFFFull));
}
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;  // splitmix64, fixed seed
static uint64_t rng() {
    rng_state += 0x9E3779B97F4A7C15ull;
    uint64_t z = rng_state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- the window predicate: biased exponent in [767, 1279]; the sign fails sqrt's and not a division's
static void window() {
    const uint64_t ones = 0xFFFFFFFFFFFFFull;
    CHECK(RG_UNSCALED_EXP_LO == 1023u - 256u && RG_UNSCALED_EXP_HI == 1023u + 256u);
    unsigned admitted = 0;
    for (unsigned e = 0; e <= 2047; ++e) {
        const bool in = e >= 767 && e <= 1279;
        for (uint64_t m : {(uint64_t)0, ones, rng() & ones, (uint64_t)1, (uint64_t)1 << 51}) {
            const double x = make(0, e, m), nx = make(1, e, m);
            CHECK(rg_unscaled_ok_hi(rg_high_dword(x)) == in);
            CHECK(!rg_unscaled_ok_hi(rg_high_dword(nx)));  // a negative operand never passes sqrt's test
            CHECK(rg_unscaled_ok_abs_hi(rg_high_dword(x)) == in);
            CHECK(rg_unscaled_ok_abs_hi(rg_high_dword(nx)) == in);
            admitted += in;
        }
    }
    CHECK(admitted == 513u * 5u);
    // the edges by value
    CHECK(rg_unscaled_ok_hi(rg_high_dword(ldexp(1.0, -256))));
    CHECK(!rg_unscaled_ok_hi(rg_high_dword(nextafter(ldexp(1.0, -256), 0.0))));
    CHECK(rg_unscaled_ok_hi(rg_high_dword(nextafter(ldexp(1.0, 257), 0.0))));
    CHECK(!rg_unscaled_ok_hi(rg_high_dword(ldexp(1.0, 257))));
    CHECK(rg_unscaled_ok_hi(rg_high_dword(1.0)) && rg_unscaled_ok_hi(rg_high_dword(1e-13 * 1e-13)));
    // the excluded classes
    const double inf = from_bits(0x7ff0000000000000ull), nan = from_bits(0x7ff8000000000000ull);
    for (double x : {0.0, -0.0, 4.9e-324, 2.2250738585072009e-308, 2.2250738585072014e-308, inf, -inf, nan, -nan,
                     from_bits(0x7ff0000000000001ull), 1e-100, 1e100, -1.0}) {
        CHECK(!rg_unscaled_ok_hi(rg_high_dword(x)));
        if (!(x == -1.0)) CHECK(!rg_unscaled_ok_abs_hi(rg_high_dword(x)));
    }
    CHECK(rg_unscaled_ok_abs_hi(rg_high_dword(-1.0)));
    // sqrt of an admitted operand is an admitted divisor; the quotient of two admitted operands is normal
    const double lo = ldexp(1.0, -256), hi = nextafter(ldexp(1.0, 257), 0.0);
    CHECK(rg_unscaled_ok_hi(rg_high_dword(sqrt(lo))) && rg_unscaled_ok_hi(rg_high_dword(sqrt(hi))));
    CHECK(lo / hi >= 2.2250738585072014e-308 && hi / lo < inf);
    std::printf("window: %u of %u exponent/mantissa samples admitted\n", admitted, 2048u * 5u);
}

int main(int argc, char **argv) {
    const bool all = argc < 2;
    if (all || !std::strcmp(argv[1], "window")) window();
    std::printf(failures ? "failed\n" : "ok\n");
    return failures ? 1 : 0;
}
