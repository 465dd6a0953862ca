// band_plan_test.cpp — the band arithmetic of the host-visible and the supersampled
// frames (raingun_amd/csrc/rg_band_plan.h) on the CPU: invariants over a grid of frame
// sizes and forced settings, and fixed values derived by hand from the formulas.
// Stand-alone; tests/test_band_plan.py builds it with AddressSanitizer + UBSan and
// runs it.  Prints "ok" and exits 0, or names the first failing check.
#include <cstdio>
#include <cstdlib>

#include "../../raingun_amd/csrc/rg_band_plan.h"

#define CHECK(cond, ...)                                             \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                \
            std::printf("\n");                                       \
            std::exit(1);                                            \
        }                                                            \
    } while (0)

// The bands tile [0, H) exactly once, in order, and none is empty.
static void check_tiling(const rg_band_plan &p, uint32_t W, uint32_t H, const char *what, int forced, uint32_t k) {
    CHECK(p.width == W && p.host_rows == H, "%s %ux%u forced %d k %u", what, W, H, forced, k);
    CHECK(p.bands >= 1 && p.band_rows >= 1, "%s %ux%u forced %d k %u", what, W, H, forced, k);
    uint64_t next = 0;
    for (uint32_t b = 0; b < p.bands; ++b) {
        const uint64_t r0 = (uint64_t)b * p.band_rows;  // where the delivery puts band b
        const uint32_t n = rg_band_rows(p, b);
        CHECK(r0 == next, "%s %ux%u forced %d k %u band %u starts at %llu, not %llu", what, W, H, forced, k, b,
              (unsigned long long)r0, (unsigned long long)next);
        CHECK(n >= 1 && n <= p.band_rows, "%s %ux%u forced %d k %u band %u has %u rows", what, W, H, forced, k, b, n);
        CHECK(n == p.band_rows || b + 1 == p.bands, "%s %ux%u forced %d k %u band %u is short (%u) and not the last",
              what, W, H, forced, k, b, n);
        next = r0 + n;
    }
    CHECK(next == H, "%s %ux%u forced %d k %u covers %llu rows", what, W, H, forced, k, (unsigned long long)next);
}

static rg_band_plan image(int forced, uint32_t W, uint32_t H) { return rg_image_band_plan(forced, W, H, RG_IMAGE_BAND_PX); }
static rg_band_plan aa(int forced, uint32_t W, uint32_t H, uint32_t k) {
    return rg_aa_band_plan(forced, W, H, k, RG_AA_SLOT_BYTES, RG_AA_MIN_BAND_ROWS);
}

int main() {
    // frames are landscape or square (W >= H); sizes around the 8-row tiles and the band thresholds
    const uint32_t Ws[] = {1, 7, 8, 9, 33, 97, 160, 800, 1920, 2048, 3840, 4096, 20000};
    const uint32_t Hs[] = {1, 2, 7, 8, 9, 15, 16, 17, 61, 63, 64, 65, 128, 243, 600, 1080, 2047, 2048, 2160, 3000};
    for (uint32_t W : Ws)
        for (uint32_t H : Hs) {
            if (W < H) continue;
            // image bands: -2 / -1 / 0 choose automatically here, 1..RG_IMAGE_MAX_BANDS are forced
            for (int forced = -2; forced <= RG_IMAGE_MAX_BANDS; ++forced) {
                const rg_band_plan p = image(forced, W, H);
                check_tiling(p, W, H, "image", forced, 1);
                CHECK(p.band_rows % 8 == 0, "image %ux%u forced %d: %u rows per band", W, H, forced, p.band_rows);
                CHECK(p.bands <= RG_IMAGE_MAX_BANDS, "image %ux%u forced %d: %u bands", W, H, forced, p.bands);
                if (forced > 0) CHECK(p.bands <= (uint32_t)forced, "image %ux%u forced %d: %u bands", W, H, forced, p.bands);
                else CHECK(p.bands <= 3, "image %ux%u automatic: %u bands", W, H, p.bands);
            }
            for (uint32_t k = 1; k <= 8; ++k)
                for (int forced : {0, 1, 7, 8, 16, 100, 70000}) {
                    const rg_band_plan p = aa(forced, W, H, k);
                    check_tiling(p, W, H, "aa", forced, k);
                    if (forced > 0) {
                        CHECK(p.band_rows == ((uint32_t)forced < H ? (uint32_t)forced : H), "aa %ux%u k %u forced %d: %u rows", W,
                              H, k, forced, p.band_rows);
                        continue;
                    }
                    const size_t scratch = (size_t)k * p.band_rows * k * W * 16;
                    CHECK(scratch <= RG_AA_SLOT_BYTES || p.band_rows <= RG_AA_MIN_BAND_ROWS, "aa %ux%u k %u: %zu B per band",
                          W, H, k, scratch);
                    CHECK(p.band_rows % 8 == 0 || p.band_rows == H, "aa %ux%u k %u: %u rows per band", W, H, k, p.band_rows);
                }
        }

    // a frame delivered whole
    const rg_band_plan one = rg_one_band(320, 88);
    check_tiling(one, 320, 88, "one", 0, 1);
    CHECK(one.bands == 1 && rg_band_rows(one, 0) == 88, "one band of 88 rows");

    // fixed values
    rg_band_plan p = image(0, 3840, 2160);  // 8294400 px / 2 Mi = 3 bands of 2160 / 3 rows
    CHECK(p.bands == 3 && p.band_rows == 720, "image 3840x2160: %u x %u", p.bands, p.band_rows);
    p = image(7, 800, 600);  // ceil(600 / 7) = 86 -> 88 rows, ceil(600 / 88) = 7
    CHECK(p.bands == 7 && p.band_rows == 88 && rg_band_rows(p, 6) == 72, "image 800x600 / 7: %u x %u", p.bands, p.band_rows);
    p = image(7, 97, 61);  // ceil(61 / 7) = 9 -> 16 rows, ceil(61 / 16) = 4
    CHECK(p.bands == 4 && p.band_rows == 16 && rg_band_rows(p, 3) == 13, "image 97x61 / 7: %u x %u", p.bands, p.band_rows);
    p = aa(0, 1920, 1080, 2);  // 64 Mi / (4 * 1920 * 16) = 546 -> 544 rows
    CHECK(p.bands == 2 && p.band_rows == 544 && rg_band_rows(p, 1) == 536, "aa 1920x1080 k 2: %u x %u", p.bands, p.band_rows);
    p = aa(0, 3840, 2160, 4);  // 64 Mi / (16 * 3840 * 16) = 68 -> 64 rows, ceil(2160 / 64) = 34
    CHECK(p.bands == 34 && p.band_rows == 64, "aa 3840x2160 k 4: %u x %u", p.bands, p.band_rows);
    p = aa(0, 3840, 2160, 8);  // 64 Mi / (64 * 3840 * 16) = 17 -> 16 rows
    CHECK(p.bands == 135 && p.band_rows == 16, "aa 3840x2160 k 8: %u x %u", p.bands, p.band_rows);
    p = aa(0, 20000, 3000, 8);  // 64 Mi / (64 * 20000 * 16) = 3 -> 0 -> the 8-row minimum
    CHECK(p.bands == 375 && p.band_rows == RG_AA_MIN_BAND_ROWS, "aa 20000x3000 k 8: %u x %u", p.bands, p.band_rows);

    std::printf("ok\n");
    return 0;
}
