// rg_render_cfg.h — what the twelve template parameters of rg_render_kernel mean, said once.
// RenderCfg<the same twelve> names every fact derived from them, for the kernel (rg_render_kernel.h),
// the launchers (rg_render_launch.h) and the grid arithmetic (rg_render_grid.h) alike;
// LightCfg / HeavyCfg and RenderCfg::staged / ::plain are how a launch site says which kernel it
// means.  The sentinel encodings of LBT and TPW are decoded (and, by the aliases, encoded) here and
// nowhere else.  Plain constants, no HIP: tests/native/render_cfg_test.cpp checks them on the CPU.
#pragma once
#include <cstdint>

#include "rg_device.h"

// ---------------------------------------------------------------- scheduling tunables
// Light path, non-persistent waves: a wave renders at most this many 8x8 tiles
// and exits, and the grid holds one wave per that many tiles, so the hardware
// dispatcher hands out CU slots wave by wave -- across the kernels of frames in
// flight too -- instead of 3072 persistent waves pinning their slots until the
// frame's queue is empty.  16 measured best for the whole 4K frame and for
// 1/2 .. 1/8 shares (profiles/r01/variants_light_tiles_per_wave.txt; 12 / 20 / 32
// re-measured in rounds 3-4: profiles/r04/s29, profiles/r04/s13).
#ifndef RG_LIGHT_TILES_PER_WAVE
#define RG_LIGHT_TILES_PER_WAVE 16
#endif
#ifndef RG_HEAVY_TILES_PER_WAVE
#define RG_HEAVY_TILES_PER_WAVE 0  // heavy path: 0 = persistent blocks (one per CU)
#endif
#ifndef RG_SHADOW_FAN
// heavy path, single small launches (TASKS): up to this many more lights of a hit traced by idle
// lanes per iteration.  Off for frames in flight and whole frames since the light buffers made
// shadow rays cheap: north star 1.594 -> 1.497 ms (8K 5.38 -> 5.06), while a 1/8 share as one
// launch keeps it (slowest share 0.648 vs 0.712 ms without; profiles/r05/s20, s21)
#define RG_SHADOW_FAN 3
#endif
#ifndef RG_HOST_RING
#define RG_HOST_RING 16  // light path into pinned host memory: tiles per queue group and ring flush (0: one store per tile)
#endif
#ifndef RG_LIGHT_BLOCK_WAVES
#define RG_LIGHT_BLOCK_WAVES 1  // light path: waves per block (blocks retire wave by wave)
#endif
#ifndef RG_HEAVY_F32_FILTER
#define RG_HEAVY_F32_FILTER true  // heavy path without a BVH: f32 pre-filter in front of the exact sphere tests
#endif

// The two parameters that carry more than a number.
// LBT: 1 is the heavy path (one ray per lane); anything else the light path with |LBT| lights per
// shadow batch -- a light batch of one is therefore written -1.
// TPW (light path): tiles a wave renders before it exits; 0 = RG_LIGHT_TILES_PER_WAVE, below 0 =
// persistent waves that take tiles until the queue is empty (single launches, whose makespan is
// their slowest wave's tile sum).
constexpr int RG_LBT_HEAVY = 1;
constexpr int RG_TPW_DEFAULT = 0, RG_TPW_PERSISTENT = -1;
// MAXD below 0: the camera family -- the MAXD == 0 kernels (frames in the launch context's global
// buffer, any depth, host-frame features) whose primary rays start at RgKernelArgs::cam_eye.
constexpr int RG_MAXD_CAMERA = -1;
// ... and RG_MAXD_LENS: the lens family -- the camera family's kernels whose primary rays leave a point of
// the launch's lens disk for the plane in focus (rg_lens.h; the bands of a supersampled frame, rg_aa.hip).
constexpr int RG_MAXD_LENS = -2;
// ... and RG_MAXD_AREA: the area family -- the lens family's kernels (the lens ray where the launch has a
// lens, the camera ray otherwise: uniform across the launch) whose spherical lights are seen at a point of
// their sphere per sample (rg_area.h; the bands of a supersampled frame of a scene with light radii).
constexpr int RG_MAXD_AREA = -3;
constexpr bool rg_lbt_light(int lbt) { return lbt != RG_LBT_HEAVY; }
constexpr int rg_lbt_of_lights(int lights) { return lights == 1 ? -1 : lights; }
// The kernel's launch bounds (its attribute stands in front of any `using K`).  Light path: blocks of
// RG_LIGHT_BLOCK_WAVES waves, at least WPS waves per SIMD (the second bound is waves per execution
// unit on AMD); heavy path: ONE block of 4 * WPS waves per CU.  Both cap the VGPRs at 512 / WPS.
constexpr int rg_block_waves(int lbt, int wps) { return rg_lbt_light(lbt) ? RG_LIGHT_BLOCK_WAVES : 4 * wps; }
constexpr int rg_min_waves_per_eu(int lbt, int wps) { return rg_lbt_light(lbt) ? wps : 1; }

// MAXD: array frames per lane (0: frames in the global buffer; RG_MAXD_CAMERA: the same, and the
// primary rays of a movable camera, rg_camera.h -- the camera family; RG_MAXD_LENS: those through a thin
// lens, rg_lens.h -- the lens family; RG_MAXD_AREA: those with area lights, rg_area.h -- the area family).  LSPH / LCOLD: which tables a block
// stages into LDS (rg_render_kernel.h).  WPS: waves per SIMD.  F32F: the f32 sphere pre-filter.  BVH:
// the sphere BVH.  TASKS: task splitting.  HF: the host-frame features with MAXD array frames.
// SPARSE: a tile list under a pixel mask.  PLAIN: scene facts compiled in.
template <int MAXD_, bool LSPH_, bool LCOLD_, int WPS_, int LBT_, bool F32F_, bool BVH_, bool TASKS_, int TPW_ = 0,
          bool HF_ = false, bool SPARSE_ = false, bool PLAIN_ = false>
struct RenderCfg {
    // the parameters as given: only launch_one's expansion into rg_render_kernel<...> reads LBT and TPW
    static constexpr int MAXD = MAXD_, WPS = WPS_, LBT = LBT_, TPW = TPW_;
    static constexpr bool LSPH = LSPH_, LCOLD = LCOLD_, F32F = F32F_, BVH = BVH_, TASKS = TASKS_, HF = HF_,
                          SPARSE = SPARSE_, PLAIN = PLAIN_;

    static constexpr bool light = rg_lbt_light(LBT);              // the light path (shadow batches), else the heavy path
    static constexpr int lights_per_batch = LBT < 0 ? -LBT : LBT;  // 1 on the heavy path
    static constexpr bool area = MAXD == RG_MAXD_AREA;            // lights with a radius (rg_area.h); a lens if the launch has one
    static constexpr bool lens = MAXD == RG_MAXD_LENS;            // ... through the launch's thin lens (rg_lens.h)
    static constexpr bool camera = MAXD == RG_MAXD_CAMERA || lens || area;  // primary rays from the launch's camera (rg_camera.h)
    static constexpr bool global_frames = MAXD == 0 || camera;    // frames in the global buffer, no per-lane array
    static constexpr int array_frames = global_frames ? 0 : MAXD;  // the lane's frame array (rg_k_frames.h FrameStack)
    // Host-frame features (deferred tile stores, tile publication, streaming cancellation, tile
    // shapes other than 8x8): the global-frame kernels, which host-visible one-launch renders use,
    // and the HF ones.  The array kernels of device-resident renders stay lean (the runtime checks
    // alone cost test1 3 %, profiles/r02/ab_hostf.txt).
    static constexpr bool host_frames = global_frames || HF;
    static constexpr bool asks_persistent = TPW < 0;
    // tiles a wave renders before it exits; 0: persistent waves
    static constexpr uint32_t tiles_per_wave = host_frames || asks_persistent ? 0u
                                               : light ? (TPW > 0 ? (uint32_t)TPW : (uint32_t)RG_LIGHT_TILES_PER_WAVE)
                                                       : (uint32_t)RG_HEAVY_TILES_PER_WAVE;
    static constexpr bool persistent = tiles_per_wave == 0;
    // light single launches of the array kernels: RG_LIGHT_PERSIST_BLOCKS_PER_CU blocks per CU (rg_render_grid.h)
    static constexpr bool light_persistent = light && !global_frames && asks_persistent;
    static constexpr int ring = host_frames && light ? RG_HOST_RING : 0;  // LDS tile ring of the light host frames (0: none)
    static constexpr bool lds_nodes_only = !LSPH && LCOLD && BVH;        // only the BVH nodes in LDS (SphNodesLds)
    // the next queue slot claimed at a tile's start: light path, device-resident, non-persistent
    static constexpr bool slot_prefetch = !host_frames && light && !asks_persistent;
    static constexpr bool shadow_fan = !light && TASKS && RG_SHADOW_FAN > 0;

    static constexpr int waves_per_block = rg_block_waves(LBT, WPS);
    static constexpr int block_threads = 64 * waves_per_block;
    static constexpr int min_waves_per_eu = rg_min_waves_per_eu(LBT, WPS);
    // the kernel's tile_px[rows][64] (a wave's finished pixels, host frames), and what of it
    // launch_waves takes from the LDS budget in front of the scene
    static constexpr int tile_px_rows = host_frames ? waves_per_block : 1;
    static constexpr uint32_t tile_px_budget_bytes = host_frames ? (uint32_t)tile_px_rows * 64u * 4u : 0u;

    static_assert(!BVH || 4 * WPS <= RG_BVH_MAX_WAVES, "one BVH stack per wave");
    static_assert(MAXD >= RG_MAXD_AREA, "MAXD: array frames, 0, RG_MAXD_CAMERA, RG_MAXD_LENS or RG_MAXD_AREA");
    static_assert(!lens || (!SPARSE && !HF), "the lens family: dense device-resident bands only");
    static_assert(!area || (!SPARSE && !HF), "the area family: dense device-resident bands only");
    static_assert(!SPARSE || (global_frames && !HF), "sparse launches run the global-frame kernels");
    static_assert(!PLAIN || (light && LSPH && LCOLD && !global_frames && !HF && !SPARSE),
                  "PLAIN: device-resident launches of the LDS-blob light kernels");

    // the same kernel with these tables staged in LDS; its PLAIN form (whole scene staged)
    template <bool S, bool C>
    using staged = RenderCfg<MAXD, S, C, WPS, LBT, F32F, BVH, TASKS, TPW, HF, SPARSE, false>;
    using plain = RenderCfg<MAXD, true, true, WPS, LBT, F32F, BVH, TASKS, TPW, HF, SPARSE, true>;
};

// What a launch site names (its staging is launch_waves' choice: K::staged, K::plain).
// Light path: exact f64 tests only, no BVH, no tasks, no HF.  LIGHTS: lights per shadow batch (1 .. RG_LB).
template <int MAXD, int WPS, int LIGHTS, int TPW = RG_TPW_DEFAULT, bool SPARSE = false>
using LightCfg = RenderCfg<MAXD, false, false, WPS, rg_lbt_of_lights(LIGHTS), false, false, false, TPW, false, SPARSE>;
// Heavy path: RG_HEAVY_WPS waves per SIMD, one ray per lane, the heavy path's own tiles per wave; the
// BVH kernels always run the f32 pre-filter.
template <int MAXD, bool BVH, bool TASKS, bool HF = false, bool SPARSE = false>
using HeavyCfg = RenderCfg<MAXD, false, false, RG_HEAVY_WPS, RG_LBT_HEAVY, BVH || RG_HEAVY_F32_FILTER, BVH, TASKS,
                           RG_TPW_DEFAULT, HF, SPARSE>;
