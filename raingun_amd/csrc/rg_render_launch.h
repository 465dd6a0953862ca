// rg_render_launch.h — launch policy of rg_render_kernel: which configuration (rg_render_cfg.h) a launch
// runs -- launch_light / launch_heavy choose the kernel, launch_waves what it stages in LDS -- and
// launch_one, which asks the occupancy, takes the grid from rg_render_grid.h and launches.
// launch_light<MAXD, SPARSE> / launch_heavy<MAXD, HF, SPARSE> are instantiated explicitly, one per
// rg_render_*.hip (SPARSE: the launches of a tile list under a pixel mask, global frames only;
// MAXD = RG_MAXD_CAMERA: the launches of a scene with a camera; MAXD = RG_MAXD_LENS: the bands of a
// supersampled frame through a thin lens; MAXD = RG_MAXD_AREA: those of a scene with light radii), so every
// rg_render_kernel instantiation is emitted by exactly one translation unit (the occupancy cache
// and the HIP runtime identify a kernel by its host address); the dispatcher (rg_kernels.hip
// dispatch_depth) sees only the declarations below.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "rg_device.h"
#include "rg_exact.h"
#include "rg_render_cfg.h"
#include "rg_render_grid.h"
#include "rg_render_kernel.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------- launchers
// Occupancy of one kernel instantiation on the current device (cached: rg_kernels.hip).
__attribute__((visibility("hidden"))) hipError_t occupancy(const void *kern, int threads, size_t lds, int &cus, int &per_cu);

// Launch (or, with grid_threads != nullptr, only size: the threads of the
// grid, which a global-frame launch needs for its frame buffer) the kernel of configuration K.
template <class K>
static hipError_t launch_one(const RgKernelArgs *a, size_t lds, hipStream_t stream, size_t *grid_threads) {
    // Block size (K::block_threads).  The heavy path shares one LDS copy of the scene (and the
    // BVH stacks / task pool) among the CU's 4*WPS waves: one block per CU.
    // The light path's scene is a few KB, so it runs small blocks, each with
    // its own copy: a block then holds its CU slot only while ITS waves work,
    // and with frames in flight the next frame's blocks take the slots of
    // waves that finished (a 4*WPS-wave block would keep the CU until its
    // slowest wave -- one refractive tile -- is done).
    auto kern = rg_render_kernel<K::MAXD, K::LSPH, K::LCOLD, K::WPS, K::LBT, K::F32F, K::BVH, K::TASKS, K::TPW, K::HF,
                                 K::SPARSE, K::PLAIN>;
    int cus = 0, per_cu = 0;
    const hipError_t oe = occupancy(reinterpret_cast<const void *>(kern), K::block_threads, lds, cus, per_cu);
    if (oe != hipSuccess) return oe;
    // sparse launches: the grid is sized from the tile list, not from the frame
    const unsigned long long tiles = K::SPARSE ? a->tile_limit : rg_tile_count(*a);
    const unsigned long long blocks = rg_render_grid_blocks<K>(tiles, cus, per_cu, a->pipelined != 0, a->max_grid_threads);
    if (grid_threads) {
        *grid_threads = (size_t)blocks * K::block_threads;
        return hipSuccess;
    }
    if (K::global_frames && (a->deep_stack == nullptr || (unsigned long long)a->deep_stride < blocks * K::block_threads))
        return hipErrorInvalidValue;  // the caller sized the frame buffer for another grid
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(K::block_threads), lds, stream, *a);
    return hipGetLastError();
}

#ifndef RG_LDS_BUDGET
#define RG_LDS_BUDGET (160 * 1024)       // one block per CU owns the CU's LDS
#endif
// RG_HEAVY_SCENE_BODIES and the path decision (rg_heavy_path) live in rg_device.h

// K with the tables staged that fit the block's LDS (K's own LSPH / LCOLD are not read).
template <class K>
static hipError_t launch_waves(const RgKernelArgs *a, hipStream_t stream, size_t *gt) {
    // the kernel's static LDS in front of the scene: the BVH kernels' per-wave traversal stacks,
    // the host frames' tile_px, the task pool
    constexpr uint32_t budget = RG_LDS_BUDGET - (K::BVH ? (uint32_t)sizeof(rg_bvh_stack) : 0u) - K::tile_px_budget_bytes -
                                (K::TASKS ? (uint32_t)sizeof(TaskPool) : 0u);
    if (a->lds_total_bytes <= budget)  // whole scene (empty sphere part if n_sph == 0)
        return launch_one<typename K::template staged<true, true>>(a, a->lds_total_bytes, stream, gt);
    if (a->n_sph > 0 && a->lds_hot_bytes <= budget)
        return launch_one<typename K::template staged<true, false>>(a, a->lds_hot_bytes, stream, gt);
    if constexpr (K::BVH) {  // the sphere tables do not fit: the BVH nodes alone, after the per-lane walk stacks
        const uint32_t nodes_lds = a->lds_lstack_bytes + (uint32_t)a->n_nodes * (uint32_t)sizeof(RgBvhNode);
        if (a->n_nodes > 0 && nodes_lds <= budget)
            return launch_one<typename K::template staged<false, true>>(a, nodes_lds, stream, gt);
    }
    return launch_one<typename K::template staged<false, false>>(a, a->lds_lstack_bytes, stream, gt);
}

#ifndef RG_LIGHT_BIG_TILES
#define RG_LIGHT_BIG_TILES 50000ull  // whole 4K frames and 1/2 shares (test1 1/2 share 0.1504 -> 0.1490 ms)
#endif
#ifndef RG_LIGHT_SINGLE_PERSISTENT
// light path: single launches run persistent waves (RG_TPW_PERSISTENT); 2: only launches below
// RG_LIGHT_BIG_TILES (rg_render_multi's shares and bands), at 2 waves per SIMD -- test1 1/8
// share 0.183 -> 0.166 ms, its 8-device rehearsal 0.3175 -> 0.297 ms (2.8x -> 3.0x); test3
// equal; 3 waves per SIMD: no gain (profiles/r04/s27/session.txt)
#define RG_LIGHT_SINGLE_PERSISTENT 2
#endif
#ifndef RG_LIGHT_WPS
#define RG_LIGHT_WPS 4            // light path: waves per SIMD (128 VGPRs; 3 -> 4: test1 -3 %, test3 -8 %, profiles/r02/ab_light_wps.txt)
#endif
#ifndef RG_LIGHT_TPW_BIG
// light path, 3-light batch: tiles per wave of whole-frame launches (0: off).  32: test1 0.2938 ->
// 0.2923 ms over 3 x 200 frames (-m gpu 284 passed, profiles/r06/s45), but 0.304 -> 0.319 ms in
// the driver's 20-frame configuration (longer waves, longer drain at the end of a short burst:
// s46), so off
#define RG_LIGHT_TPW_BIG 0
#endif
#ifndef RG_LIGHT_WPS_ONE
#define RG_LIGHT_WPS_ONE RG_LIGHT_WPS  // the one-light batch (118 VGPRs at 4 waves per SIMD)
#endif

// The light-batch ladder: a light scene runs the kernels of the narrowest shadow batch that is
// switched on and holds its lights -- one light (RG_LB_ONE), RG_LB_SMALL, RG_LB -- at that step's
// waves per SIMD.  f(step) is called with the scene's step.
template <int LIGHTS, int WPS>
struct LightStep {
    static constexpr int lights = LIGHTS, wps = WPS;
};
template <class F>
static inline auto rg_light_ladder(int n_lights, F &&f) {
    static_assert(RG_LB_SMALL < RG_LB, "RG_LB is the ladder's last and widest step (launch_light tells it by its width)");
    if constexpr (RG_LB_ONE != 0) {  // a light, or none: a batch of one
        if (n_lights <= 1) return f(LightStep<1, RG_LIGHT_WPS_ONE>{});
    }
    if constexpr (RG_LB_SMALL > 1) {
        // a batch that wide, not RG_LB (the per-light loops of the shadow batch are unrolled over
        // the batch; test3's one light: 0.2525 -> 0.2293 ms at 2, profiles/r06/s24)
        if (n_lights <= RG_LB_SMALL) return f(LightStep<RG_LB_SMALL, RG_LIGHT_WPS>{});
    }
    return f(LightStep<RG_LB, RG_LIGHT_WPS>{});
}

// Lights per shadow batch of the light kernel that a scene with n_lights lights runs.
static inline int rg_light_batch(int n_lights) {
    return rg_light_ladder(n_lights, [](auto step) { return decltype(step)::lights; });
}

// May a device-resident light launch run the PLAIN instantiation of its kernel (rg_render_kernel.h)?  Every
// fact that kernel holds at compile time, checked here: no disks and no boxes, no f32 RGB output, no
// tile order, no light buffers, no NaN-scene path, a shadow batch exactly as wide as the scene's light
// count -- and the whole scene in LDS (the PLAIN kernels are LSPH && LCOLD ones).  And what their
// camera ray relies on (rg_exact.h): the launch context's sweep of this frame size found the
// reciprocal form of the camera quotients equal to the division for every column and row,
// and it has the arena's device image with their two tables (plain_veto: a word it writes, not the
// frame's size), and the ray's squared length stays in the range where sqrt and the reciprocal need
// no scaling.
static inline bool rg_light_plain(const RgKernelArgs &a) {
    return a.n_dsk == 0 && a.n_box == 0 && a.rgb == nullptr && a.tile_perm == nullptr && a.lbuf == nullptr &&
           a.nan_scene == 0 && a.n_lights == rg_light_batch(a.n_lights) && a.lds_total_bytes <= RG_LDS_BUDGET &&
           a.lds_plain_bytes <= RG_LDS_BUDGET && a.plain_veto == 0 && rg_camera_unscaled_ok(a.fov_adjustment, a.aspect);
}

// One light launch: the PLAIN kernel where the launch admits it (array frames only), else launch_waves' choice.
template <class K>
static hipError_t launch_light_one(const RgKernelArgs *a, hipStream_t stream, size_t *gt, bool plain) {
    if constexpr (!K::global_frames)
        if (plain) return launch_one<typename K::plain>(a, a->lds_plain_bytes, stream, gt);  // with its two tables
    return launch_waves<K>(a, stream, gt);
}

// Light scenes (few bodies): per-iteration overhead dominates -> fewer,
// fatter iterations (a batch of shadow rays per pass) at RG_LIGHT_WPS waves/SIMD.  Heavy
// scenes: the body loop dominates and waves mix ray kinds -> one ray per
// lane in ONE shared loop, RG_HEAVY_WPS waves/SIMD to hide LDS/FP64 latency.
// ran_plain (nullable): set to 1 when the launch runs a PLAIN instantiation, else to 0.
template <int MAXD, bool SPARSE = false>
__attribute__((visibility("hidden"))) hipError_t launch_light(const RgKernelArgs *a, hipStream_t stream, size_t *gt,
                                                              int *ran_plain) {
    const bool plain = MAXD > 0 && !SPARSE && rg_light_plain(*a);
    if (ran_plain) *ran_plain = plain ? 1 : 0;
    return rg_light_ladder(a->n_lights, [&](auto step) -> hipError_t {
        using S = decltype(step);
        if constexpr (SPARSE) {  // global frames: one kernel per step
            return launch_waves<LightCfg<MAXD, S::wps, S::lights, RG_TPW_DEFAULT, true>>(a, stream, gt);
        } else {
            // a launch on its own (not one of several frames in flight): persistent waves at full
            // occupancy balance the tiles dynamically, where a fixed tiles-per-wave grid makes every
            // wave render exactly that many tiles and the slowest wave's sum the makespan
            // (2: launches below RG_LIGHT_BIG_TILES tiles only -- rg_render_multi's shares and bands)
            if constexpr (MAXD > 0 && RG_LIGHT_SINGLE_PERSISTENT != 0) {
                if (!a->pipelined && (RG_LIGHT_SINGLE_PERSISTENT != 2 || rg_tile_count(*a) < RG_LIGHT_BIG_TILES))
                    return launch_light_one<LightCfg<MAXD, S::wps, S::lights, RG_TPW_PERSISTENT>>(a, stream, gt, plain);
            }
#if RG_LIGHT_TPW_BIG > 0
            // whole frames (frames in flight): RG_LIGHT_TPW_BIG tiles per wave, half the waves of
            // RG_LIGHT_TILES_PER_WAVE (as a compile-time variant: test1 0.2968 -> 0.2943 ms over 200
            // frames, profiles/r06/s43); smaller launches (the 1/N shares) keep 16
            if constexpr (MAXD > 0 && S::lights == RG_LB) {
                if (rg_tile_count(*a) >= RG_LIGHT_BIG_TILES)
                    return launch_light_one<LightCfg<MAXD, S::wps, S::lights, RG_LIGHT_TPW_BIG>>(a, stream, gt, plain);
            }
#endif
            return launch_light_one<LightCfg<MAXD, S::wps, S::lights>>(a, stream, gt, plain);
        }
    });
}

#ifndef RG_HEAVY_TASKS
#define RG_HEAVY_TASKS 1   // task splitting on the heavy path, for launches of fewer than RG_HEAVY_TASK_TILES tiles
#endif
#ifndef RG_HEAVY_TASK_TILES
// Task splitting shortens the slowest pixels' ray trees, which bound a small
// launch; on a large one (and with frames in flight, whose next frame fills
// the tail) its bookkeeping costs more than it saves: with 4 frames in flight
// synth1024 4K 3.10 -> 2.88 ms and 8K 11.18 -> 9.94 ms without it, but a 1/8
// share (16k tiles) 0.538 -> 0.561 ms (profiles/r01/variants_heavy_tasks.txt)
#define RG_HEAVY_TASK_TILES 24576
#endif

template <int MAXD, bool HF = false, bool SPARSE = false>
__attribute__((visibility("hidden"))) hipError_t launch_heavy(const RgKernelArgs *a, hipStream_t stream, size_t *gt) {
    const unsigned long long tiles = SPARSE ? a->tile_limit : rg_tile_count(*a);
    // frames in flight (pipelined): the throughput-sized grid already keeps blocks long;
    // task splitting then costs more than it saves (1/8 share 0.400 -> 0.384 ms without:
    // profiles/r02/ab_task_split.txt); a single small launch keeps it (its latency)
    const bool tasks = RG_HEAVY_TASKS && tiles < RG_HEAVY_TASK_TILES && !a->pipelined;
    constexpr bool BVH = true, TASKS = true;
    if (a->n_nodes > 0)
        return tasks ? launch_waves<HeavyCfg<MAXD, BVH, TASKS, HF, SPARSE>>(a, stream, gt)
                     : launch_waves<HeavyCfg<MAXD, BVH, !TASKS, HF, SPARSE>>(a, stream, gt);
    return tasks ? launch_waves<HeavyCfg<MAXD, !BVH, TASKS, HF, SPARSE>>(a, stream, gt)
                 : launch_waves<HeavyCfg<MAXD, !BVH, !TASKS, HF, SPARSE>>(a, stream, gt);
}

// one explicit instantiation each, in the rg_render_*.hip of that name
extern template hipError_t launch_light<8>(const RgKernelArgs *, hipStream_t, size_t *, int *);
extern template hipError_t launch_light<16>(const RgKernelArgs *, hipStream_t, size_t *, int *);
extern template hipError_t launch_light<64>(const RgKernelArgs *, hipStream_t, size_t *, int *);
extern template hipError_t launch_light<0>(const RgKernelArgs *, hipStream_t, size_t *, int *);
extern template hipError_t launch_heavy<8, false>(const RgKernelArgs *, hipStream_t, size_t *);
extern template hipError_t launch_heavy<16, false>(const RgKernelArgs *, hipStream_t, size_t *);
extern template hipError_t launch_heavy<64, false>(const RgKernelArgs *, hipStream_t, size_t *);
extern template hipError_t launch_heavy<0, false>(const RgKernelArgs *, hipStream_t, size_t *);
extern template hipError_t launch_heavy<8, true>(const RgKernelArgs *, hipStream_t, size_t *);
extern template hipError_t launch_light<0, true>(const RgKernelArgs *, hipStream_t, size_t *, int *);
extern template hipError_t launch_heavy<0, false, true>(const RgKernelArgs *, hipStream_t, size_t *);
// the camera family (rg_render_*_camera*.hip): dense and sparse, light and heavy
extern template hipError_t launch_light<RG_MAXD_CAMERA>(const RgKernelArgs *, hipStream_t, size_t *, int *);
extern template hipError_t launch_heavy<RG_MAXD_CAMERA, false>(const RgKernelArgs *, hipStream_t, size_t *);
extern template hipError_t launch_light<RG_MAXD_CAMERA, true>(const RgKernelArgs *, hipStream_t, size_t *, int *);
extern template hipError_t launch_heavy<RG_MAXD_CAMERA, false, true>(const RgKernelArgs *, hipStream_t, size_t *);
// the lens family (rg_render_*_lens.hip): dense only, light and heavy
extern template hipError_t launch_light<RG_MAXD_LENS>(const RgKernelArgs *, hipStream_t, size_t *, int *);
extern template hipError_t launch_heavy<RG_MAXD_LENS, false>(const RgKernelArgs *, hipStream_t, size_t *);
// the area family (rg_render_*_area.hip): dense only, light and heavy
extern template hipError_t launch_light<RG_MAXD_AREA>(const RgKernelArgs *, hipStream_t, size_t *, int *);
extern template hipError_t launch_heavy<RG_MAXD_AREA, false>(const RgKernelArgs *, hipStream_t, size_t *);
