// tile_deal_test.cpp — the dealing of tiles to ranks and devices, the part and slot sizes, the
// re-interleave's source rows and the direct-mode bands of rg_render_multi
// (raingun_amd/csrc/rg_tile_deal.h) on the CPU: invariants over a grid of heights, tile rows,
// worlds, root shares and band settings, and fixed values derived by hand from the formulas.
// Stand-alone; tests/test_tile_deal.py builds it with AddressSanitizer + UBSan and runs it.
// Prints "ok" and exits 0, or names the first failing check.  With an argument it prints the
// deal of a fixed list of cases instead, which the Python test compares with
// raingun_amd/distributed.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../raingun_amd/csrc/rg_tile_deal.h"

#define CHECK(cond, ...)                                             \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                \
            std::printf("\n");                                       \
            std::exit(1);                                            \
        }                                                            \
    } while (0)

// The render kernel's "i-th selected tile -> image tile" (out_row_to_y, rg_k_frames.h), restated.
static unsigned long long kernel_tile(const rg_tiling &t, uint32_t group, uint32_t sel) {
    const unsigned long long i = sel;
    return group > 1u ? (i / group) * t.tile_stride + t.tile_offset + i % group : i * t.tile_stride + t.tile_offset;
}

static void check_deal(uint32_t H, uint32_t T, uint32_t world, uint32_t root) {
    const rg_deal d{T, world, root};
    const uint32_t tiles = rg_deal_image_tiles(d, H);
#define WF "H %u T %u world %u root %u"
#define WA H, T, world, root
    CHECK((unsigned long long)tiles * T >= H && (unsigned long long)(tiles - 1) * T < H, WF, WA);
    // 1. every tile has one owner; within an owner the indices count up from 0 in increasing t
    std::vector<uint32_t> count(world, 0);
    for (uint32_t t = 0; t < tiles; ++t) {
        const rg_deal_place o = rg_deal_tile(d, t);
        CHECK(o.rank < world, WF, WA);
        CHECK(o.at == count[o.rank], WF ": tile %u is rank %u's %u-th, after %u", WA, t, o.rank, o.at, count[o.rank]);
        ++count[o.rank];
    }
    uint32_t most_sent = 0;  // the largest part that travels in the gather
    for (uint32_t r = 0; r < world; ++r) {
        CHECK(rg_deal_rank_tiles(d, H, r) == count[r], WF ": rank %u: %u, counted %u", WA, r, rg_deal_rank_tiles(d, H, r),
              count[r]);
        // 2. the rank's launch, enumerated as the kernel does, visits its tiles in part order
        const rg_tiling tl = rg_deal_tiling(d, r);
        const uint32_t group = rg_deal_group(d, r);
        CHECK(rg_tiling_valid(&tl) && tl.tile_rows == T, WF, WA);
        for (uint32_t i = 0; i < count[r]; ++i) {
            const unsigned long long t = kernel_tile(tl, group, i);
            CHECK(t < tiles, WF ": rank %u selected tile %u is image tile %llu", WA, r, i, t);
            const rg_deal_place o = rg_deal_tile(d, (uint32_t)t);
            CHECK(o.rank == r && o.at == i, WF ": rank %u selected tile %u -> image tile %llu -> rank %u's %u", WA, r, i, t,
                  o.rank, o.at);
        }
        CHECK(kernel_tile(tl, group, count[r]) >= tiles, WF ": rank %u has a tile more", WA, r);
        // 3. rows
        CHECK(rg_tiling_rows_grouped(H, &tl, group) == count[r] * T, WF, WA);
        CHECK(rg_deal_part_rows(d, H, r) == count[r] * T, WF, WA);
        // root 1: every rank's part travels in an equal slot (rank 0's too); root > 1: rank 0's does not
        if (r > 0 || root == 1) most_sent = std::max(most_sent, count[r]);
    }
    CHECK(rg_deal_slot_rows(d, H) == most_sent * T, WF ": slot %u rows, most tiles sent %u", WA, rg_deal_slot_rows(d, H),
          most_sent);
    // 4. every image row comes from inside its rank's part, and no two from the same place
    std::vector<std::vector<char>> seen(world);
    for (uint32_t r = 0; r < world; ++r) seen[r].assign((size_t)count[r] * T, 0);
    for (uint32_t y = 0; y < H; ++y) {
        const rg_deal_place o = rg_deal_source_row(d, y);
        CHECK(o.rank < world && o.at < count[o.rank] * T, WF ": row %u from rank %u row %u", WA, y, o.rank, o.at);
        CHECK(!seen[o.rank][o.at], WF ": row %u: rank %u row %u read twice", WA, y, o.rank, o.at);
        seen[o.rank][o.at] = 1;
        const rg_deal_place tile = rg_deal_tile(d, y / T);
        CHECK(o.rank == tile.rank && o.at == tile.at * T + y % T, WF ": row %u", WA, y);
    }
#undef WF
#undef WA
}

static void check_direct(uint32_t W, uint32_t H, uint32_t T, int n, int forced) {
#define WF "%ux%u T %u n %d forced %d"
#define WA W, H, T, n, forced
    const rg_multi_plan p = rg_multi_band_plan(W, H, T, n, forced);
    const rg_deal d{T, (uint32_t)n, 1u};
    CHECK(p.tiles == rg_deal_image_tiles(d, H) && p.per_dev == rg_deal_rank_tiles(d, H, 0), WF, WA);
    CHECK(p.K >= 1 && p.K <= RG_MULTI_MAX_BANDS && p.J >= 1, WF ": K %d J %u", WA, p.K, p.J);
    CHECK(forced <= 0 || p.K <= forced, WF ": K %d", WA, p.K);
    std::vector<int> band_of(H, -1);  // the band whose copy wrote the row
    for (int i = 0; i < n; ++i) {
        const uint32_t sel = rg_deal_rank_tiles(d, H, (uint32_t)i);
        uint32_t next = 0;
        for (int b = 0; b < p.K; ++b) {
            const rg_multi_band c = rg_multi_band_of(p, (uint32_t)i, (uint32_t)b);
            // 5. the bands cut [0, sel) once and in order
            CHECK(c.j0 == next && c.j1 >= c.j0 && c.j1 <= sel, WF ": device %d band %d: [%u, %u) after %u of %u", WA, i, b, c.j0,
                  c.j1, next, sel);
            next = c.j1;
            if (i == 0) CHECK(c.j1 > c.j0, WF ": device 0 band %d is empty", WA, b);
            if (c.j1 == c.j0) continue;
            CHECK(c.full + (c.has_partial ? 1u : 0u) == c.j1 - c.j0, WF ": device %d band %d", WA, i, b);
            // 6. the copies: part row (j - j0) T + r of the band is row r of the device's tile j
            auto write = [&](size_t y, uint32_t j, uint32_t r) {
                CHECK(y < H, WF ": device %d band %d writes row %zu", WA, i, b, y);
                CHECK(band_of[y] < 0, WF ": device %d band %d writes row %zu again", WA, i, b, y);
                band_of[y] = b;
                const rg_deal_place o = rg_deal_source_row(d, (uint32_t)y);
                CHECK(o.rank == (uint32_t)i && o.at == j * T + r, WF ": device %d band %d row %zu is tile %u row %u", WA, i, b,
                      y, j, r);
            };
            for (uint32_t k = 0; k < c.full; ++k)  // the strided copy: T rows every n T rows
                for (uint32_t r = 0; r < T; ++r) write(c.dst_row + ((size_t)k * n) * T + r, c.j0 + k, r);
            if (c.has_partial) {
                CHECK(c.partial_rows >= 1 && c.partial_rows < T, WF ": device %d band %d", WA, i, b);
                for (uint32_t r = 0; r < c.partial_rows; ++r) write(c.partial_row + r, c.j0 + c.full, r);
            }
        }
        CHECK(next == sel, WF ": device %d: bands cover %u of %u tiles", WA, i, next, sel);
    }
    // 7. band b's pageable range holds rows of band-b copies only; the ranges tile [0, H)
    size_t at = 0;
    for (int b = 0; b < p.K; ++b) {
        const rg_row_range y = rg_multi_band_rows(p, (uint32_t)b);
        CHECK(y.y0 == at && y.y1 >= y.y0 && y.y1 <= H, WF ": band %d rows [%zu, %zu) after %zu", WA, b, y.y0, y.y1, at);
        for (size_t r = y.y0; r < y.y1; ++r) CHECK(band_of[r] == b, WF ": row %zu in band %d's range, written by %d", WA, r, b, band_of[r]);
        at = y.y1;
    }
    CHECK(at == H, WF ": the ranges cover %zu rows", WA, at);  // with 6.: every row written exactly once
#undef WF
#undef WA
}

// (H, T, world, root) whose deal the Python test compares with distributed.py
static const uint32_t kCases[][4] = {{1, 8, 1, 1},   {357, 8, 8, 1},  {357, 8, 8, 2},  {243, 8, 3, 3},  {149, 16, 2, 4},
                                     {61, 8, 8, 2},  {61, 8, 8, 1},   {40, 8, 2, 1},   {17, 16, 9, 4},  {2160, 16, 8, 3},
                                     {130, 4, 5, 2}, {129, 1, 9, 4},  {9, 8, 2, 1},    {9, 8, 3, 2},    {7, 8, 4, 4}};

static int print_cases() {
    for (const auto &c : kCases) {
        const uint32_t H = c[0];
        const rg_deal d{c[1], c[2], c[3]};
        std::printf("case %u %u %u %u slot %u\n", H, d.T, d.world, d.root, rg_deal_slot_rows(d, H));
        std::vector<std::vector<uint32_t>> of(d.world);
        for (uint32_t t = 0; t < rg_deal_image_tiles(d, H); ++t) of[rg_deal_tile(d, t).rank].push_back(t);
        for (uint32_t r = 0; r < d.world; ++r) {
            std::printf("rank %u:", r);
            for (uint32_t t : of[r]) std::printf(" %u", t);
            std::printf("\n");
        }
    }
    return 0;
}

int main(int argc, char **) {
    if (argc > 1) return print_cases();

    std::vector<uint32_t> Hs;
    for (uint32_t h = 1; h <= 130; ++h) Hs.push_back(h);
    for (uint32_t h : {243u, 357u, 2160u}) Hs.push_back(h);
    const uint32_t Ts[] = {1, 4, 8, 16};
    for (uint32_t H : Hs)
        for (uint32_t T : Ts)
            for (uint32_t world = 1; world <= 9; ++world) {
                // shares with no tiles at all (tiles < world) are in here
                for (uint32_t root = 1; root <= (world > 1 ? 4u : 1u); ++root) check_deal(H, T, world, root);
                const int n = (int)world;
                for (int forced = 1; forced <= 4; ++forced) check_direct(640, H, T, n, forced);
                check_direct(640, H, T, n, 0);
                // automatic: the widths at which a share reaches k Mi pixels, and the largest below
                for (unsigned long long k = 2; k <= 4; ++k) {
                    const unsigned long long at = ((k << 20) * n + H - 1) / H, below = (((k << 20) - 1) * n) / H;
                    CHECK(rg_multi_bands(0, (uint32_t)at, H, n) == (int)k, "%llux%u n %d", at, H, n);
                    CHECK(rg_multi_bands(0, (uint32_t)below, H, n) == (int)k - 1, "%llux%u n %d", below, H, n);
                    check_direct((uint32_t)at, H, T, n, 0);
                    check_direct((uint32_t)below, H, T, n, 0);
                }
            }

    // fixed values, by hand
    // 357 rows in tiles of 8: 45 tiles, the last of 5 rows; 8 ranks, root 2: periods of 9, 5 whole periods
    rg_deal d{8, 8, 2};
    CHECK(rg_deal_image_tiles(d, 357) == 45, "tiles");
    CHECK(rg_deal_part_rows(d, 357, 0) == 80 && rg_deal_part_rows(d, 357, 7) == 40 && rg_deal_slot_rows(d, 357) == 40, "rows");
    rg_deal_place o = rg_deal_tile(d, 44);  // 44 = 4 * 9 + 8: the period's tile 8 is rank 8 - 2 + 1
    CHECK(o.rank == 7 && o.at == 4, "tile 44: rank %u at %u", o.rank, o.at);
    o = rg_deal_tile(d, 10);  // 10 = 1 * 9 + 1: rank 0's 1 * 2 + 1
    CHECK(o.rank == 0 && o.at == 3, "tile 10: rank %u at %u", o.rank, o.at);
    o = rg_deal_source_row(d, 85);  // tile 10, row 5 of it
    CHECK(o.rank == 0 && o.at == 29, "row 85: rank %u row %u", o.rank, o.at);
    o = rg_deal_source_row(d, 356);  // tile 44, row 4 of it
    CHECK(o.rank == 7 && o.at == 36, "row 356: rank %u row %u", o.rank, o.at);
    rg_tiling tl = rg_deal_tiling(d, 3);
    CHECK(tl.tile_rows == 8 && tl.tile_stride == 9 && tl.tile_offset == 4 && rg_deal_group(d, 3) == 1, "rank 3's tiling");
    tl = rg_deal_tiling(d, 0);
    CHECK(tl.tile_stride == 9 && tl.tile_offset == 0 && rg_deal_group(d, 0) == 2, "rank 0's tiling");
    d = {8, 8, 1};  // round robin: ceil(45 / 8) = 6 tiles
    CHECK(rg_deal_slot_rows(d, 357) == 48 && rg_deal_part_rows(d, 357, 5) == 40, "round robin rows");
    d = {8, 3, 3};  // 243 rows: 31 tiles = 6 periods of 5 and one tile more, rank 0's
    CHECK(rg_deal_part_rows(d, 243, 0) == 152 && rg_deal_slot_rows(d, 243) == 48, "243 rows, world 3, root 3");
    d = {16, 2, 4};  // 149 rows: 10 tiles = 2 periods of 5
    CHECK(rg_deal_part_rows(d, 149, 0) == 128 && rg_deal_slot_rows(d, 149) == 32, "149 rows, world 2, root 4");
    CHECK(rg_packed_slot_bytes(48, 97) == 13968, "48 x 97 x 3 = 13968 = 873 x 16");
    CHECK(rg_packed_slot_bytes(40, 97) == 11648, "40 x 97 x 3 = 11640 -> 728 x 16");
    tl = {8, 9, 0};
    CHECK(rg_tiling_rows_grouped(357, &tl, 10) == 0, "a group larger than the stride");
    tl = {8, 9, 9};
    CHECK(!rg_tiling_valid(&tl) && rg_tiling_rows_grouped(357, &tl, 1) == 0, "offset == stride");

    // rg_render_multi on 8 devices, 640 x 357, T = 8: 45 tiles, 6 on devices 0..4 and 5 on 5..7; the
    // partial tile 44 is device 4's tile 5.  A share is 28560 pixels: automatically one band
    rg_multi_plan p = rg_multi_band_plan(640, 357, 8, 8, 0);
    CHECK(p.tiles == 45 && p.per_dev == 6 && p.J == 6 && p.K == 1, "bands 0: J %u K %d", p.J, p.K);
    rg_multi_band c = rg_multi_band_of(p, 4, 0);
    CHECK(c.j0 == 0 && c.j1 == 6 && c.full == 5 && c.has_partial && c.dst_row == 32 && c.partial_row == 352 &&
              c.partial_rows == 5, "bands 0, device 4");
    rg_row_range y = rg_multi_band_rows(p, 0);  // 6 * 8 * 8 = 384 rows, cut at 357
    CHECK(y.y0 == 0 && y.y1 == 357, "bands 0: rows [%zu, %zu)", y.y0, y.y1);
    p = rg_multi_band_plan(640, 357, 8, 8, 3);  // 3 bands of 2 tiles
    CHECK(p.J == 2 && p.K == 3, "bands 3: J %u K %d", p.J, p.K);
    c = rg_multi_band_of(p, 4, 2);  // tiles 4, 5 = image tiles 36, 44
    CHECK(c.j0 == 4 && c.j1 == 6 && c.full == 1 && c.has_partial && c.dst_row == 288 && c.partial_row == 352 &&
              c.partial_rows == 5, "bands 3, device 4, band 2");
    c = rg_multi_band_of(p, 5, 2);  // tile 4 = image tile 37, its last
    CHECK(c.j0 == 4 && c.j1 == 5 && c.full == 1 && !c.has_partial && c.dst_row == 296, "bands 3, device 5, band 2");
    c = rg_multi_band_of(p, 7, 0);
    CHECK(c.j0 == 0 && c.j1 == 2 && c.full == 2 && !c.has_partial && c.dst_row == 56, "bands 3, device 7, band 0");
    y = rg_multi_band_rows(p, 1);  // 2 * 8 * 8 = 128 rows per band
    CHECK(y.y0 == 128 && y.y1 == 256, "bands 3, band 1: rows [%zu, %zu)", y.y0, y.y1);
    y = rg_multi_band_rows(p, 2);
    CHECK(y.y0 == 256 && y.y1 == 357, "bands 3, band 2: rows [%zu, %zu)", y.y0, y.y1);
    p = rg_multi_band_plan(640, 357, 8, 8, 4);  // ceil(6 / 4) = 2 tiles per band: 3 bands cover 6
    CHECK(p.J == 2 && p.K == 3, "bands 4: J %u K %d", p.J, p.K);
    // 4K: 8294400 pixels; / 2^20 = 7.9 on one device (the cap), 3.96 on two, 0.99 on eight
    CHECK(rg_multi_bands(0, 3840, 2160, 1) == 4 && rg_multi_bands(0, 3840, 2160, 2) == 3 &&
              rg_multi_bands(0, 3840, 2160, 8) == 1 && rg_multi_bands(9, 3840, 2160, 8) == 4, "automatic bands at 4K");

    std::printf("ok\n");
    return 0;
}
