// The area family's configuration (raingun_amd/csrc/rg_render_cfg.h: MAXD = RG_MAXD_AREA): what RenderCfg
// decodes from it -- K::area, which implies K::camera but not K::lens (the lens ray is the launch's choice) --
// that it is the camera family's kernel in every other derived fact, its grid, and that the area table's
// pointer lies in the lens's padding: RgKernelArgs keeps its size and every offset.  A stand-alone host
// program like tests/native/lens_cfg_test.cpp (tests/test_area_cpu.py compiles it host-only; no kernel is
// instantiated, no HIP call made).
#include <cstddef>
#include <cstdio>
#include <type_traits>

#include "../../raingun_amd/csrc/rg_render_launch.h"

static_assert(RG_MAXD_AREA == -3 && RG_MAXD_LENS == -2 && RG_MAXD_CAMERA == -1);

template <class A, class C>
constexpr bool same_but_area() {
    return A::area && !C::area && !A::lens && A::camera && C::camera && A::global_frames && C::global_frames &&
           A::array_frames == 0 && A::light == C::light && A::lights_per_batch == C::lights_per_batch &&
           A::host_frames == C::host_frames && A::persistent == C::persistent && A::tiles_per_wave == C::tiles_per_wave &&
           A::light_persistent == C::light_persistent && A::ring == C::ring && A::lds_nodes_only == C::lds_nodes_only &&
           A::slot_prefetch == C::slot_prefetch && A::shadow_fan == C::shadow_fan && A::block_threads == C::block_threads &&
           A::min_waves_per_eu == C::min_waves_per_eu && A::tile_px_rows == C::tile_px_rows &&
           A::tile_px_budget_bytes == C::tile_px_budget_bytes && !A::SPARSE && !A::PLAIN && !A::HF;
}

using LightArea = LightCfg<RG_MAXD_AREA, 4, 3>::staged<true, true>;
static_assert(std::is_same_v<LightArea, RenderCfg<-3, true, true, 4, 3, false, false, false, 0, false, false, false>>);
static_assert(same_but_area<LightArea, LightCfg<RG_MAXD_CAMERA, 4, 3>::staged<true, true>>());
static_assert(same_but_area<LightCfg<RG_MAXD_AREA, 4, 1>, LightCfg<RG_MAXD_CAMERA, 4, 1>>());
using HeavyArea = HeavyCfg<RG_MAXD_AREA, true, true>::staged<false, true>;
static_assert(same_but_area<HeavyArea, HeavyCfg<RG_MAXD_CAMERA, true, true>::staged<false, true>>());
static_assert(same_but_area<HeavyCfg<RG_MAXD_AREA, false, false>, HeavyCfg<RG_MAXD_CAMERA, false, false>>());
static_assert(HeavyArea::shadow_fan && HeavyArea::TASKS);  // the sites that trace for another lane's pixel exist in it
// no other kernel is an area kernel
static_assert(!LightCfg<RG_MAXD_LENS, 4, 3>::area && !LightCfg<RG_MAXD_CAMERA, 4, 3>::area && !LightCfg<0, 4, 3>::area &&
              !LightCfg<8, 4, 3>::area && !HeavyCfg<64, true, false>::area && !HeavyCfg<0, false, false, false, true>::area);
// the table's pointer is the lens's padding: the struct the parent's kernels read is the struct they read before
static_assert(offsetof(RgKernelArgs, area_tab) == offsetof(RgKernelArgs, lens_pad) && sizeof(const double *) == sizeof(uint32_t[2]));
static_assert(offsetof(RgKernelArgs, area_tab) == offsetof(RgKernelArgs, lens_tab) + sizeof(const double *));
static_assert(sizeof(RgKernelArgs) == offsetof(RgKernelArgs, area_tab) + sizeof(const double *));

int main() {
    int failures = 0;
    // the family's grid is the camera kernel's (the launch context sizes the frame buffer from it)
    for (unsigned long long tiles : {1ull, 63ull, 4096ull, 129600ull})
        for (int per_cu : {1, 2, 8, 16})
            for (bool pipelined : {false, true})
                for (unsigned long long cap : {0ull, 4096ull}) {
                    if (rg_render_grid_blocks<LightArea>(tiles, 8, per_cu, pipelined, cap) !=
                        rg_render_grid_blocks<LightCfg<RG_MAXD_CAMERA, 4, 3>::staged<true, true>>(tiles, 8, per_cu, pipelined, cap))
                        ++failures;
                    if (rg_render_grid_blocks<HeavyArea>(tiles, 8, per_cu, pipelined, cap) !=
                        rg_render_grid_blocks<HeavyCfg<RG_MAXD_CAMERA, true, true>::staged<false, true>>(tiles, 8, per_cu, pipelined, cap))
                        ++failures;
                }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::puts("ok");
    return 0;
}
