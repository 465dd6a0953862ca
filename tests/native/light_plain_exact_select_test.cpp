// What the PLAIN selection predicate (raingun_amd/csrc/rg_render_launch.h rg_light_plain) gained with the
// exact-division kernels (rg_exact.h), over hand-built RgKernelArgs: a stand-alone host program
// (tests/test_exact_div.py compiles it host-only; no kernel is instantiated, no HIP call made).
// The conditions it had before: tests/native/light_plain_select_test.cpp.
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../raingun_amd/csrc/rg_render_launch.h"

static int failures = 0;
#define CHECK(cond)                                               \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            ++failures;                                           \
        }                                                         \
    } while (0)

// test1 at 4K as rg_launch_tiles fills it (fov 90 degrees)
static RgKernelArgs plain_args(int n_lights) {
    RgKernelArgs a;
    std::memset(&a, 0, sizeof a);
    a.n_sph = 4;
    a.n_pln = 2;
    a.n_bodies = 6;
    a.n_lights = n_lights;
    a.n_textures = 2;
    a.path = RG_PATH_AUTO;
    a.lds_total_bytes = 2048;
    a.lds_plain_bytes = 2048 + 2 * sizeof(RgTexMagic) + 6 * sizeof(RgPlnAxes);
    a.width = 3840;
    a.height = 2160;
    a.width_d = 3840.0;
    a.height_d = 2160.0;
    a.inv_w = 1.0 / 3840.0;
    a.inv_h = 1.0 / 2160.0;
    a.aspect = 3840.0 / 2160.0;
    a.fov_adjustment = 1.0;
    a.max_depth = 5;
    return a;
}

int main() {
    for (int n = 1; n <= 3; ++n) {
        const RgKernelArgs ok = plain_args(n);
        CHECK(rg_light_plain(ok));
        RgKernelArgs a = ok;
        a.plain_veto = 1;  // the quotient sweep failed for this frame size (or is switched off)
        CHECK(!rg_light_plain(a));
        a.plain_veto = 2;  // no blob image: the two tables are nowhere
        CHECK(!rg_light_plain(a));
        a = ok;
        a.lds_plain_bytes = RG_LDS_BUDGET + 16;  // the arena fits, its two extra tables do not
        CHECK(!rg_light_plain(a));
        a.lds_plain_bytes = RG_LDS_BUDGET;
        CHECK(rg_light_plain(a));
        // the camera ray's range: 1 + fa^2 (1 + aspect^2) <= 2^100, and no NaN
        a = ok;
        a.fov_adjustment = 114.58865012930961;  // 179 degrees
        a.aspect = 512.0;                       // 4096 x 8
        CHECK(rg_light_plain(a));
        a.fov_adjustment = 1e15;
        CHECK(!rg_light_plain(a));
        a = ok;
        a.aspect = 1e16;
        CHECK(!rg_light_plain(a));
        a = ok;
        a.fov_adjustment = std::numeric_limits<double>::quiet_NaN();
        CHECK(!rg_light_plain(a));
        a = ok;
        a.fov_adjustment = std::numeric_limits<double>::infinity();
        CHECK(!rg_light_plain(a));
        // what it still must not look at: the frame's size and tiling, the reciprocals themselves
        a = ok;
        a.width = 97;
        a.height = 61;
        a.inv_w = 0.0;
        a.inv_h = 0.0;
        a.tile_stride = 8;
        a.tile_offset = 7;
        a.rows_identity = 0;
        a.tile_rows_shift = 32;
        CHECK(rg_light_plain(a));
    }
    std::printf(failures ? "failed\n" : "ok\n");
    return failures ? 1 : 0;
}
