// The camera family's configuration (raingun_amd/csrc/rg_render_cfg.h: MAXD = RG_MAXD_CAMERA): what
// RenderCfg decodes from it, that it is the MAXD == 0 kernel in every other derived fact, and its
// grid.  A stand-alone host program like tests/native/render_cfg_test.cpp (tests/test_camera_cpu.py
// compiles it host-only; no kernel is instantiated, no HIP call made).
#include <cstdio>
#include <type_traits>

#include "../../raingun_amd/csrc/rg_render_launch.h"

static_assert(RG_MAXD_CAMERA == -1);

template <class C, class Z>
constexpr bool same_but_camera() {
    return C::camera && !Z::camera && C::global_frames && Z::global_frames && C::array_frames == 0 && Z::array_frames == 0 &&
           C::light == Z::light && C::lights_per_batch == Z::lights_per_batch && C::host_frames == Z::host_frames &&
           C::persistent == Z::persistent && C::tiles_per_wave == Z::tiles_per_wave &&
           C::light_persistent == Z::light_persistent && C::ring == Z::ring && C::lds_nodes_only == Z::lds_nodes_only &&
           C::slot_prefetch == Z::slot_prefetch && C::shadow_fan == Z::shadow_fan && C::block_threads == Z::block_threads &&
           C::min_waves_per_eu == Z::min_waves_per_eu && C::tile_px_rows == Z::tile_px_rows &&
           C::tile_px_budget_bytes == Z::tile_px_budget_bytes && C::SPARSE == Z::SPARSE && !C::PLAIN && !C::HF;
}

using LightCam = LightCfg<RG_MAXD_CAMERA, 4, 3>::staged<true, true>;
static_assert(std::is_same_v<LightCam, RenderCfg<-1, true, true, 4, 3, false, false, false, 0, false, false, false>>);
static_assert(same_but_camera<LightCam, LightCfg<0, 4, 3>::staged<true, true>>());
static_assert(LightCam::host_frames && LightCam::persistent && LightCam::ring == RG_HOST_RING);
static_assert(same_but_camera<LightCfg<RG_MAXD_CAMERA, 4, 1, RG_TPW_DEFAULT, true>, LightCfg<0, 4, 1, RG_TPW_DEFAULT, true>>());
using HeavyCam = HeavyCfg<RG_MAXD_CAMERA, true, true>::staged<false, true>;
static_assert(same_but_camera<HeavyCam, HeavyCfg<0, true, true>::staged<false, true>>());
static_assert(HeavyCam::lds_nodes_only && HeavyCam::shadow_fan && HeavyCam::block_threads == 256 * RG_HEAVY_WPS);
static_assert(same_but_camera<HeavyCfg<RG_MAXD_CAMERA, false, false, false, true>, HeavyCfg<0, false, false, false, true>>());
// the array kernels are no cameras, and their frame array keeps its size
static_assert(!LightCfg<8, 4, 3>::camera && LightCfg<8, 4, 3>::array_frames == 8 && !LightCfg<8, 4, 3>::global_frames);
static_assert(!HeavyCfg<64, true, false>::camera && HeavyCfg<64, true, false>::array_frames == 64);

int main() {
    int failures = 0;
    // the family's grid is the MAXD == 0 kernel's (the launch context sizes the frame buffer from it)
    for (unsigned long long tiles : {1ull, 63ull, 4096ull, 129600ull})
        for (int per_cu : {1, 2, 8, 16})
            for (bool pipelined : {false, true})
                for (unsigned long long cap : {0ull, 4096ull}) {
                    if (rg_render_grid_blocks<LightCam>(tiles, 8, per_cu, pipelined, cap) !=
                        rg_render_grid_blocks<LightCfg<0, 4, 3>::staged<true, true>>(tiles, 8, per_cu, pipelined, cap))
                        ++failures;
                    if (rg_render_grid_blocks<HeavyCam>(tiles, 8, per_cu, pipelined, cap) !=
                        rg_render_grid_blocks<HeavyCfg<0, true, true>::staged<false, true>>(tiles, 8, per_cu, pipelined, cap))
                        ++failures;
                }
    // a camera launch sets the PLAIN veto (rg_launch.hip), and a vetoed launch is never PLAIN
    RgKernelArgs a = {};
    a.n_lights = 3;
    a.fov_adjustment = 1.0;
    a.aspect = 16.0 / 9.0;
    if (!rg_light_plain(a)) ++failures;
    a.plain_veto = 4u;
    if (rg_light_plain(a)) ++failures;
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::puts("ok");
    return 0;
}
