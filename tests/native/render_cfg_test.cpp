// The render kernel's configuration (raingun_amd/csrc/rg_render_cfg.h RenderCfg and the aliases the
// launch sites use), the grid arithmetic (rg_render_grid.h) and the light-batch ladder
// (rg_render_launch.h): a stand-alone host program (tests/test_render_cfg.py compiles it host-only;
// no kernel is instantiated, no HIP call made).  The grid cases are worked by hand from the rules
// rg_render_grid.h states, with 8 CUs; the figures assume the default tunables (RG_HEAVY_WPS 3,
// RG_LIGHT_WPS 4, 16 light tiles per wave, RG_HOST_RING 16).
#include <cstdio>
#include <type_traits>

#include "../../raingun_amd/csrc/rg_render_launch.h"

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);        \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// ---------------------------------------------------------------- one kernel of each kind
// heavy: BVH scene, task splitting, the whole scene staged
using Heavy = HeavyCfg<8, true, true>::staged<true, true>;
static_assert(std::is_same_v<Heavy, RenderCfg<8, true, true, 3, 1, true, true, true, 0, false, false, false>>);
static_assert(!Heavy::light && Heavy::lights_per_batch == 1);
static_assert(Heavy::block_threads == 768 && Heavy::waves_per_block == 12 && Heavy::min_waves_per_eu == 1);
static_assert(Heavy::persistent && Heavy::tiles_per_wave == 0 && !Heavy::light_persistent);
static_assert(!Heavy::global_frames && !Heavy::host_frames && Heavy::ring == 0);
static_assert(Heavy::tile_px_rows == 1 && Heavy::tile_px_budget_bytes == 0);
static_assert(Heavy::shadow_fan && !Heavy::slot_prefetch && !Heavy::lds_nodes_only);
static_assert(HeavyCfg<8, true, true>::staged<false, true>::lds_nodes_only);   // only the BVH nodes staged
static_assert(!HeavyCfg<8, false, true>::staged<false, true>::lds_nodes_only);  // no BVH: nothing of the kind
static_assert(!HeavyCfg<8, true, false>::shadow_fan);                           // the fan belongs to task splitting
// heavy host-frame: array frames with the host-frame features, no BVH
using HeavyHost = HeavyCfg<8, false, false, true>::staged<true, false>;
static_assert(std::is_same_v<HeavyHost, RenderCfg<8, true, false, 3, 1, true, false, false, 0, true, false, false>>);
static_assert(!HeavyHost::light && !HeavyHost::global_frames && HeavyHost::host_frames && HeavyHost::persistent);
static_assert(HeavyHost::ring == 0 && HeavyHost::tile_px_rows == 12 && HeavyHost::tile_px_budget_bytes == 12 * 64 * 4);
// light default: three lights, 16 tiles per wave
using Light = LightCfg<8, 4, 3>::staged<true, true>;
static_assert(std::is_same_v<Light, RenderCfg<8, true, true, 4, 3, false, false, false, 0, false, false, false>>);
static_assert(Light::light && Light::lights_per_batch == 3);
static_assert(Light::block_threads == 64 && Light::waves_per_block == 1 && Light::min_waves_per_eu == 4);
static_assert(!Light::persistent && Light::tiles_per_wave == 16 && !Light::light_persistent && Light::slot_prefetch);
static_assert(!Light::host_frames && Light::ring == 0 && Light::tile_px_budget_bytes == 0 && !Light::shadow_fan);
static_assert(LightCfg<8, 4, 3, 32>::tiles_per_wave == 32);
// light persistent
using LightPers = LightCfg<8, 4, 3, RG_TPW_PERSISTENT>::staged<true, true>;
static_assert(std::is_same_v<LightPers, RenderCfg<8, true, true, 4, 3, false, false, false, -1, false, false, false>>);
static_assert(LightPers::light && LightPers::persistent && LightPers::tiles_per_wave == 0);
static_assert(LightPers::light_persistent && !LightPers::slot_prefetch && LightPers::block_threads == 64);
// light one-light: a batch of one is not the heavy path
using LightOne = LightCfg<8, 4, 1>::staged<true, true>;
static_assert(std::is_same_v<LightOne, RenderCfg<8, true, true, 4, -1, false, false, false, 0, false, false, false>>);
static_assert(LightOne::light && LightOne::lights_per_batch == 1 && LightOne::block_threads == 64);
static_assert(LightOne::min_waves_per_eu == 4 && LightOne::tiles_per_wave == 16 && LightOne::slot_prefetch);
// light global frames: the host-frame features and the tile ring, persistent whatever TPW says
using LightG = LightCfg<0, 4, 3>::staged<true, true>;
static_assert(LightG::light && LightG::global_frames && LightG::host_frames && LightG::ring == 16);
static_assert(LightG::persistent && !LightG::light_persistent && !LightG::slot_prefetch);
static_assert(LightG::tile_px_rows == 1 && LightG::tile_px_budget_bytes == 256);
// sparse
using Sparse = LightCfg<0, 4, 2, RG_TPW_DEFAULT, true>::staged<true, true>;
static_assert(std::is_same_v<Sparse, RenderCfg<0, true, true, 4, 2, false, false, false, 0, false, true, false>>);
static_assert(Sparse::SPARSE && Sparse::light && Sparse::lights_per_batch == 2 && Sparse::host_frames && Sparse::persistent);
using HeavySparse = HeavyCfg<0, false, true, false, true>;
static_assert(HeavySparse::SPARSE && !HeavySparse::light && HeavySparse::host_frames && HeavySparse::tile_px_rows == 12);
// PLAIN: the whole scene staged, whatever the site's staging said
using Plain = LightCfg<8, 4, 3>::plain;
static_assert(std::is_same_v<Plain, RenderCfg<8, true, true, 4, 3, false, false, false, 0, false, false, true>>);
static_assert(std::is_same_v<Plain, Light::plain>);
static_assert(Plain::PLAIN && Plain::light && Plain::tiles_per_wave == 16 && Plain::slot_prefetch && !Plain::host_frames);
static_assert(std::is_same_v<LightPers::plain, RenderCfg<8, true, true, 4, 3, false, false, false, -1, false, false, true>>);

// ---------------------------------------------------------------- the grid
constexpr unsigned long long NONE = 0;  // no max_grid_threads
template <class K>
static unsigned long long grid(unsigned long long tiles, int per_cu, bool pipelined = false, unsigned long long max_threads = NONE,
                               int cus = 8) {
    return rg_render_grid_blocks<K>(tiles, cus, per_cu, pipelined, max_threads);
}

int main() {
    // light, array frames, default tiles per wave: one 64-thread block per 16 tiles, whatever the occupancy
    for (int per_cu : {1, 4, 10, 32}) {
        CHECK(grid<Light>(1, per_cu) == 1);
        CHECK(grid<Light>(16, per_cu) == 1);
        CHECK(grid<Light>(17, per_cu) == 2);
        CHECK(grid<Light>(129600, per_cu) == 8100);
        CHECK(grid<Light>(1000, per_cu, false, 128) == 2);
        CHECK(grid<Light>(1000, per_cu, false, 32) == 1);  // the floor
        CHECK(grid<Plain>(129600, per_cu) == 8100);
        CHECK(grid<LightOne>(17, per_cu) == 2);
        CHECK(grid<Light>(129600, per_cu, true) == 8100);  // frames in flight change nothing on the light path
    }
    // light persistent
    CHECK(grid<LightPers>(1000, 10) == 48);  // clamped to 6 blocks per CU
    CHECK(grid<LightPers>(1000, 4) == 32);
    CHECK(grid<LightPers>(5, 10) == 5);
    // light global frames
    CHECK(grid<LightG>(1000, 10) == 64);  // clamped to 8 blocks per CU
    CHECK(grid<LightG>(10, 10) == 10);
    CHECK(grid<Sparse>(1000, 10) == 64);
    // heavy: 768-thread blocks of 12 waves, 1 block per CU
    CHECK(grid<Heavy>(1000, 1) == 8);
    CHECK(grid<Heavy>(13, 1) == 2);
    CHECK(grid<Heavy>(100000, 1, true) == 8);
    CHECK(grid<Heavy>(1000, 1, true) == 2);
    CHECK(grid<Heavy>(100, 1, true) == 2);  // the floor of a quarter of the blocks
    CHECK(grid<HeavyHost>(100, 1, true) == 2);
    CHECK(grid<HeavySparse>(100, 1, true) == 8);  // global frames: no pipelined cap
    CHECK(grid<Heavy>(1000, 1, false, 768 * 3 + 5) == 3);
    CHECK(grid<Heavy>(0, 1) == 1);
    static_assert(rg_render_grid_blocks<LightPers>(1000, 8, 10, false, 0) == 48, "usable in constant expressions");

    // the light-batch ladder: the step (lights, waves per SIMD) a scene with n lights runs
    const auto step = [](int n) { return rg_light_ladder(n, [](auto s) { return decltype(s)::lights * 100 + decltype(s)::wps; }); };
    CHECK(step(0) == 100 + RG_LIGHT_WPS_ONE);
    CHECK(step(1) == 100 + RG_LIGHT_WPS_ONE);
    CHECK(step(2) == 200 + RG_LIGHT_WPS);
    CHECK(step(3) == 300 + RG_LIGHT_WPS);
    for (int n = 0; n <= 3; ++n) CHECK(step(n) / 100 == rg_light_batch(n));
    std::printf(failures ? "failed\n" : "ok\n");
    return failures ? 1 : 0;
}
