// The lens family's configuration (raingun_amd/csrc/rg_render_cfg.h: MAXD = RG_MAXD_LENS): what RenderCfg
// decodes from it -- K::lens, which implies K::camera -- that it is the camera family's kernel in every
// other derived fact, its grid, and where the lens fields of RgKernelArgs lie.  A stand-alone host program
// like tests/native/camera_cfg_test.cpp (tests/test_lens_cpu.py compiles it host-only; no kernel is
// instantiated, no HIP call made).
#include <cstddef>
#include <cstdio>
#include <type_traits>

#include "../../raingun_amd/csrc/rg_render_launch.h"

static_assert(RG_MAXD_LENS == -2 && RG_MAXD_CAMERA == -1);

template <class L, class C>
constexpr bool same_but_lens() {
    return L::lens && !C::lens && L::camera && C::camera && L::global_frames && C::global_frames && L::array_frames == 0 &&
           L::light == C::light && L::lights_per_batch == C::lights_per_batch && L::host_frames == C::host_frames &&
           L::persistent == C::persistent && L::tiles_per_wave == C::tiles_per_wave &&
           L::light_persistent == C::light_persistent && L::ring == C::ring && L::lds_nodes_only == C::lds_nodes_only &&
           L::slot_prefetch == C::slot_prefetch && L::shadow_fan == C::shadow_fan && L::block_threads == C::block_threads &&
           L::min_waves_per_eu == C::min_waves_per_eu && L::tile_px_rows == C::tile_px_rows &&
           L::tile_px_budget_bytes == C::tile_px_budget_bytes && !L::SPARSE && !L::PLAIN && !L::HF;
}

using LightLens = LightCfg<RG_MAXD_LENS, 4, 3>::staged<true, true>;
static_assert(std::is_same_v<LightLens, RenderCfg<-2, true, true, 4, 3, false, false, false, 0, false, false, false>>);
static_assert(same_but_lens<LightLens, LightCfg<RG_MAXD_CAMERA, 4, 3>::staged<true, true>>());
static_assert(same_but_lens<LightCfg<RG_MAXD_LENS, 4, 1>, LightCfg<RG_MAXD_CAMERA, 4, 1>>());
using HeavyLens = HeavyCfg<RG_MAXD_LENS, true, true>::staged<false, true>;
static_assert(same_but_lens<HeavyLens, HeavyCfg<RG_MAXD_CAMERA, true, true>::staged<false, true>>());
static_assert(same_but_lens<HeavyCfg<RG_MAXD_LENS, false, false>, HeavyCfg<RG_MAXD_CAMERA, false, false>>());
// no other kernel is a lens kernel
static_assert(!LightCfg<RG_MAXD_CAMERA, 4, 3>::lens && !LightCfg<0, 4, 3>::lens && !LightCfg<8, 4, 3>::lens &&
              !HeavyCfg<64, true, false>::lens && !HeavyCfg<0, false, false, false, true>::lens);
// the lens fields stand behind everything the parent's kernels read, and the struct grew by a multiple of
// 16 bytes: the arguments that follow it in other kernels keep their 16-byte phase
static_assert(offsetof(RgKernelArgs, lens) == offsetof(RgKernelArgs, shvol_pad) + sizeof(uint32_t[3]));
static_assert(sizeof(RgKernelArgs) - offsetof(RgKernelArgs, lens) == 80 && 80 % 16 == 0);

int main() {
    int failures = 0;
    // the family's grid is the camera kernel's (the launch context sizes the frame buffer from it)
    for (unsigned long long tiles : {1ull, 63ull, 4096ull, 129600ull})
        for (int per_cu : {1, 2, 8, 16})
            for (bool pipelined : {false, true})
                for (unsigned long long cap : {0ull, 4096ull}) {
                    if (rg_render_grid_blocks<LightLens>(tiles, 8, per_cu, pipelined, cap) !=
                        rg_render_grid_blocks<LightCfg<RG_MAXD_CAMERA, 4, 3>::staged<true, true>>(tiles, 8, per_cu, pipelined, cap))
                        ++failures;
                    if (rg_render_grid_blocks<HeavyLens>(tiles, 8, per_cu, pipelined, cap) !=
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
