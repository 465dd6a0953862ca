// The PLAIN selection predicate of the light launcher (raingun_amd/csrc/rg_render_launch.h
// rg_light_plain, rg_light_batch) over hand-built RgKernelArgs: a stand-alone host program
// (tests/test_light_plain_select.py compiles it host-only; no kernel is instantiated, no HIP call made).
#include <cstdio>
#include <cstring>

#include "../../raingun_amd/csrc/rg_render_launch.h"

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);        \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// a launch every PLAIN condition holds for: test1's shape (2 planes, 4 spheres, 3 lights)
static RgKernelArgs plain_args(int n_lights) {
    RgKernelArgs a;
    std::memset(&a, 0, sizeof a);
    a.n_sph = 4;
    a.n_pln = 2;
    a.n_bodies = 6;
    a.n_lights = n_lights;
    a.path = RG_PATH_AUTO;
    a.lds_total_bytes = 2048;
    a.width = 3840;
    a.height = 2160;
    a.max_depth = 5;
    return a;
}

int main() {
    static uint32_t word;
    static float fword;
    for (int n = 1; n <= 3; ++n) {  // LB 1 (the one-light batch), 2 and 3
        const RgKernelArgs ok = plain_args(n);
        CHECK(rg_light_batch(n) == n);
        CHECK(rg_light_plain(ok));
        RgKernelArgs a = ok;  // each condition flipped once
        a.n_dsk = 1;
        CHECK(!rg_light_plain(a));
        a = ok;
        a.n_box = 1;
        CHECK(!rg_light_plain(a));
        a = ok;
        a.rgb = &fword;
        CHECK(!rg_light_plain(a));
        a = ok;
        a.tile_perm = &word;
        CHECK(!rg_light_plain(a));
        a = ok;
        a.lbuf = reinterpret_cast<const RgLightBufDev *>(&word);
        CHECK(!rg_light_plain(a));
        a = ok;
        a.nan_scene = 1;
        CHECK(!rg_light_plain(a));
        a = ok;
        a.lds_total_bytes = RG_LDS_BUDGET + 16;  // the scene does not fit LDS whole: no LSPH && LCOLD kernel
        CHECK(!rg_light_plain(a));
        a.lds_total_bytes = RG_LDS_BUDGET;
        CHECK(rg_light_plain(a));
        // what the predicate must NOT look at: the frame, the depth, frames in flight
        a = ok;
        a.width = 97;
        a.height = 61;
        a.max_depth = 0;
        a.pipelined = 1;
        CHECK(rg_light_plain(a));
    }
    // the batch must be exactly as wide as the light count: no lights runs the one-light batch
    // with an empty slot, more lights than RG_LB are the heavy path's
    CHECK(rg_light_batch(0) == 1);
    CHECK(!rg_light_plain(plain_args(0)));
    CHECK(rg_light_batch(4) == RG_LB);
    CHECK(!rg_light_plain(plain_args(4)));
    CHECK(rg_heavy_path(plain_args(4)));
    std::printf(failures ? "failed\n" : "ok\n");
    return failures ? 1 : 0;
}
