// sample_tiles_test.cpp — raingun_amd/csrc/rg_sample_tiles.h against brute force: for every
// 8x8 sample tile of every band, the output pixels it overlaps (found by walking the tile's
// samples one by one) and "listed iff some overlapped pixel is flagged" on seeded masks.
// Stand-alone (tests/test_aa_adaptive_cpu.py builds it with ASan + UBSan); prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../raingun_amd/csrc/rg_band_plan.h"
#include "../../raingun_amd/csrc/rg_sample_tiles.h"

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

int main() {
    unsigned long long tiles_checked = 0, partial_bands = 0;
    for (uint32_t k = 1; k <= 8; ++k)
        for (uint32_t W : {1u, 5u, 64u, 101u})
            for (uint32_t band_rows : {7u, 8u, 16u})
                for (uint32_t H : {1u, band_rows, 2 * band_rows + 3, 37u}) {
                    const rg_band_plan p = rg_aa_band_plan((int)band_rows, W, H, k, RG_AA_SLOT_BYTES, RG_AA_MIN_BAND_ROWS);
                    for (int density : {0, 1, 2}) {  // no pixel, about 1 in 16, every pixel flagged
                        std::vector<uint8_t> mask((size_t)W * H);
                        for (auto &m : mask) m = density == 2 || (density == 1 && rnd() % 16 == 0) ? 1 : 0;
                        for (uint32_t b = 0; b < p.bands; ++b) {
                            const uint32_t rows = rg_band_rows(p, b), r0 = b * p.band_rows;
                            if (rows != p.band_rows) ++partial_bands;
                            const uint32_t tiles_x = rg_sample_tiles_x(W, k), n = rg_sample_tile_count(W, rows, k);
                            CHECK(tiles_x == (k * W + 7) / 8);
                            CHECK(n == tiles_x * ((k * rows + 7) / 8));
                            CHECK(n <= rg_sample_tile_count(W, p.band_rows, k));  // a full band's list holds it
                            std::vector<uint32_t> owner((size_t)k * W * k * rows, 0xFFFFFFFFu);
                            for (uint32_t t = 0; t < n; ++t) {
                                const uint32_t ty = t / tiles_x, tx = t % tiles_x;
                                uint32_t x0 = ~0u, x1 = 0, y0 = ~0u, y1 = 0;
                                bool any = false, samples = false;
                                for (uint32_t sy = 8 * ty; sy < 8 * ty + 8 && sy < k * rows; ++sy)
                                    for (uint32_t sx = 8 * tx; sx < 8 * tx + 8 && sx < k * W; ++sx) {
                                        samples = true;
                                        CHECK(owner[(size_t)sy * k * W + sx] == 0xFFFFFFFFu);
                                        owner[(size_t)sy * k * W + sx] = t;
                                        const uint32_t px = sx / k, py = sy / k;
                                        x0 = px < x0 ? px : x0; x1 = px + 1 > x1 ? px + 1 : x1;
                                        y0 = py < y0 ? py : y0; y1 = py + 1 > y1 ? py + 1 : y1;
                                        any = any || mask[(size_t)(r0 + py) * W + px] != 0;
                                    }
                                CHECK(samples);  // every counted tile holds a sample of the band
                                const rg_px_rect r = rg_sample_tile_pixels(t, W, rows, k);
                                CHECK(r.x0 == x0 && r.x1 == x1 && r.y0 == y0 && r.y1 == y1);
                                CHECK(r.x1 <= W && r.y1 <= rows);
                                CHECK(rg_sample_tile_listed(mask.data() + (size_t)r0 * W, t, W, rows, k) == any);
                                ++tiles_checked;
                            }
                            for (uint32_t o : owner) CHECK(o != 0xFFFFFFFFu);  // the tiles cover the band's samples
                        }
                    }
                }
    CHECK(partial_bands > 0);
    std::printf("%llu tiles, %llu partial bands\nok\n", tiles_checked, partial_bands);
    return 0;
}
