// rg_render_launch.h — launch policy of rg_render_kernel: which instantiation a launch runs and
// with what grid.  launch_light<MAXD, SPARSE> / launch_heavy<MAXD, HF, SPARSE> are instantiated explicitly, one
// per rg_render_*.hip (SPARSE: the launches of a tile list under a pixel mask, MAXD == 0 only), so every rg_render_kernel instantiation is emitted by exactly one
// translation unit (the occupancy cache and the HIP runtime identify a kernel by its host
// address); the dispatcher (rg_kernels.hip dispatch_depth) sees only the declarations below.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "rg_device.h"
#include "rg_render_kernel.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------- launchers
// One persistent block per CU slot: grid = CUs x (blocks per CU the register
// and LDS budgets admit), capped by the tiles the frame has.
#ifndef RG_LIGHT_PERSIST_BLOCKS_PER_CU
// light persistent launches: one-wave blocks per CU (8 -> 6 once they stopped prefetching tile slots:
// test1 slowest 1/8 share 0.162-0.166 -> 0.153-0.156 ms, test3 0.139 -> 0.133; 4: 0.159, 12/16: slower;
// profiles/r05/s34, s35)
#define RG_LIGHT_PERSIST_BLOCKS_PER_CU 6
#endif
#ifndef RG_DEEP_BLOCKS_PER_CU
#define RG_DEEP_BLOCKS_PER_CU 8  // deep-stack light launches: resident one-wave blocks per CU (bounds the frame buffer)
#endif

// Occupancy of one kernel instantiation on the current device (cached: rg_kernels.hip).
__attribute__((visibility("hidden"))) hipError_t occupancy(const void *kern, int threads, size_t lds, int &cus, int &per_cu);

// Launch (or, with grid_threads != nullptr, only size: the threads of the
// grid, which a MAXD == 0 launch needs for its frame buffer) one instantiation.
template <int MAXD, bool LSPH, bool LCOLD, int WPS, int LB, bool F32F, bool BVH, bool TASKS, int TPW = 0, bool HF = false,
          bool SPARSE = false, bool PLAIN = false>
static hipError_t launch_one(const RgKernelArgs *a, size_t lds, hipStream_t stream, size_t *grid_threads) {
    // Block size.  The heavy path shares one LDS copy of the scene (and the
    // BVH stacks / task pool) among the CU's 4*WPS waves: one block per CU.
    // The light path's scene is a few KB, so it runs small blocks, each with
    // its own copy: a block then holds its CU slot only while ITS waves work,
    // and with frames in flight the next frame's blocks take the slots of
    // waves that finished (a 4*WPS-wave block would keep the CU until its
    // slowest wave -- one refractive tile -- is done).
    constexpr int threads = LB != 1 ? 64 * RG_LIGHT_BLOCK_WAVES : 256 * WPS;  // LB != 1: the light path
    auto kern = rg_render_kernel<MAXD, LSPH, LCOLD, WPS, LB, F32F, BVH, TASKS, TPW, HF, SPARSE, PLAIN>;
    int cus = 0, per_cu = 0;
    const hipError_t oe = occupancy(reinterpret_cast<const void *>(kern), threads, lds, cus, per_cu);
    if (oe != hipSuccess) return oe;
    if ((MAXD == 0 || HF) && LB != 1 && per_cu > RG_DEEP_BLOCKS_PER_CU) per_cu = RG_DEEP_BLOCKS_PER_CU;
    // light single launches, persistent waves (TPW < 0): RG_LIGHT_PERSIST_BLOCKS_PER_CU one-wave
    // blocks per CU (2 per SIMD), never more than the occupancy query admits (a scene whose LDS
    // copy allows fewer would otherwise start the extra blocks only after the queue drained)
    if (MAXD != 0 && LB != 1 && TPW < 0) per_cu = std::min(per_cu, RG_LIGHT_PERSIST_BLOCKS_PER_CU);
    // sparse launches: the grid is sized from the tile list, not from the frame
    const unsigned long long tiles = SPARSE ? a->tile_limit : rg_tile_count(*a);
    const unsigned long long waves = (unsigned long long)threads / 64u;
    unsigned long long blocks = (unsigned long long)cus * per_cu;
    const unsigned long long need = (tiles + waves - 1) / waves;
    if (blocks > need) blocks = need;
    if (LB == 1 && MAXD != 0 && a->pipelined) {
        // Heavy path, frames in flight: each persistent block takes >= RG_PIPE_TILES_PER_WAVE
        // tiles per wave, so its lifetime dwarfs its start (LDS staging) and its slowest
        // wave's tail, while every launch keeps >= 1/RG_PIPE_MIN_CU_DIV of the CUs; the other frames in
        // flight fill the rest.  North-star 1/8 share 0.440 -> 0.399 ms, 1/4 0.753 ->
        // 0.713, 8K 1/8 1.250 -> 1.220; whole frames unchanged (profiles/r02/ab_pipe_blocks.txt)
        const unsigned long long per = waves * RG_PIPE_TILES_PER_WAVE;
        unsigned long long cap = (tiles + per - 1) / per;
        const unsigned long long floor_blocks = ((unsigned long long)cus * per_cu + RG_PIPE_MIN_CU_DIV - 1) / RG_PIPE_MIN_CU_DIV;
        if (cap < floor_blocks) cap = floor_blocks;
        if (blocks > cap) blocks = cap;
    }
    constexpr unsigned long long kmax = MAXD == 0 || HF || TPW < 0 ? 0 : LB != 1 ? (TPW > 0 ? TPW : RG_LIGHT_TILES_PER_WAVE) : RG_HEAVY_TILES_PER_WAVE;
    if constexpr (kmax > 0)  // non-persistent: one wave per kmax tiles
        blocks = (tiles + waves * kmax - 1) / (waves * kmax);
    if (a->max_grid_threads && blocks * threads > a->max_grid_threads) blocks = a->max_grid_threads / threads;
    if (blocks < 1) blocks = 1;
    if (grid_threads) {
        *grid_threads = (size_t)blocks * threads;
        return hipSuccess;
    }
    if (MAXD == 0 && (a->deep_stack == nullptr || (unsigned long long)a->deep_stride < blocks * threads))
        return hipErrorInvalidValue;  // the caller sized the frame buffer for another grid
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(threads), lds, stream, *a);
    return hipGetLastError();
}

#ifndef RG_LDS_BUDGET
#define RG_LDS_BUDGET (160 * 1024)       // one block per CU owns the CU's LDS
#endif
#ifndef RG_HEAVY_F32_FILTER
#define RG_HEAVY_F32_FILTER true  // heavy path: f32 pre-filter in front of the exact sphere tests
#endif
// RG_HEAVY_SCENE_BODIES and the path decision (rg_heavy_path) live in rg_device.h

template <int MAXD, int WPS, int LB, bool F32F, bool BVH, bool TASKS, int TPW = 0, bool HF = false, bool SPARSE = false>
static hipError_t launch_waves(const RgKernelArgs *a, hipStream_t stream, size_t *gt) {
    // the BVH kernels also hold the static per-wave traversal stacks
    constexpr uint32_t budget = RG_LDS_BUDGET - (BVH ? (uint32_t)sizeof(rg_bvh_stack) : 0u) -
                                (uint32_t)(MAXD != 0 && !HF ? 0 : (LB != 1 ? RG_LIGHT_BLOCK_WAVES : 4 * WPS) * 64 * 4) -  // tile_px
                                (TASKS ? (uint32_t)sizeof(TaskPool) : 0u);
    if (a->lds_total_bytes <= budget)  // whole scene (empty sphere part if n_sph == 0)
        return launch_one<MAXD, true, true, WPS, LB, F32F, BVH, TASKS, TPW, HF, SPARSE>(a, a->lds_total_bytes, stream, gt);
    if (a->n_sph > 0 && a->lds_hot_bytes <= budget)
        return launch_one<MAXD, true, false, WPS, LB, F32F, BVH, TASKS, TPW, HF, SPARSE>(a, a->lds_hot_bytes, stream, gt);
    if constexpr (BVH) {  // the sphere tables do not fit: the BVH nodes alone, after the per-lane walk stacks
        const uint32_t nodes_lds = a->lds_lstack_bytes + (uint32_t)a->n_nodes * (uint32_t)sizeof(RgBvhNode);
        if (a->n_nodes > 0 && nodes_lds <= budget)
            return launch_one<MAXD, false, true, WPS, LB, F32F, BVH, TASKS, TPW, HF, SPARSE>(a, nodes_lds, stream, gt);
    }
    return launch_one<MAXD, false, false, WPS, LB, F32F, BVH, TASKS, TPW, HF, SPARSE>(a, a->lds_lstack_bytes, stream, gt);
}

#ifndef RG_LIGHT_BIG_TILES
#define RG_LIGHT_BIG_TILES 50000ull  // whole 4K frames and 1/2 shares (test1 1/2 share 0.1504 -> 0.1490 ms)
#endif
#ifndef RG_LIGHT_SINGLE_PERSISTENT
// light path: single launches run persistent waves (TPW < 0); 2: only launches below
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

// Lights per shadow batch of the light kernel that a scene with n_lights lights runs (launch_light below).
static inline int rg_light_batch(int n_lights) {
#if RG_LB_ONE
    if (n_lights <= 1) return 1;
#endif
#if RG_LB_SMALL > 1
    if (n_lights <= RG_LB_SMALL) return RG_LB_SMALL;
#endif
    return RG_LB;
}

// May a device-resident light launch run the PLAIN instantiation of its kernel (rg_render_kernel.h)?  Every
// fact that kernel holds at compile time, checked here: no disks and no boxes, no f32 RGB output, no
// tile order, no light buffers, no NaN-scene path, a shadow batch exactly as wide as the scene's light
// count -- and the whole scene in LDS (the PLAIN kernels are LSPH && LCOLD ones).
static inline bool rg_light_plain(const RgKernelArgs &a) {
    return a.n_dsk == 0 && a.n_box == 0 && a.rgb == nullptr && a.tile_perm == nullptr && a.lbuf == nullptr &&
           a.nan_scene == 0 && a.n_lights == rg_light_batch(a.n_lights) && a.lds_total_bytes <= RG_LDS_BUDGET;
}

// One light launch: the PLAIN kernel where the launch admits it (array frames only), else launch_waves' choice.
template <int MAXD, int WPS, int LB, int TPW>
static hipError_t launch_light_one(const RgKernelArgs *a, hipStream_t stream, size_t *gt, bool plain) {
    if constexpr (MAXD != 0)
        if (plain)
            return launch_one<MAXD, true, true, WPS, LB, false, false, false, TPW, false, false, true>(a, a->lds_total_bytes, stream, gt);
    return launch_waves<MAXD, WPS, LB, false, false, false, TPW>(a, stream, gt);
}

// Light scenes (few bodies): per-iteration overhead dominates -> fewer,
// fatter iterations (RG_LB shadow rays per pass) at 2 waves/SIMD.  Heavy
// scenes: the body loop dominates and waves mix ray kinds -> one ray per
// lane in ONE shared loop, 4 waves/SIMD to hide LDS/FP64 latency.
// ran_plain (nullable): set to 1 when the launch runs a PLAIN instantiation, else to 0.
template <int MAXD, bool SPARSE = false>
__attribute__((visibility("hidden"))) hipError_t launch_light(const RgKernelArgs *a, hipStream_t stream, size_t *gt,
                                                              int *ran_plain) {
    const bool plain = MAXD != 0 && !SPARSE && rg_light_plain(*a);
    if (ran_plain) *ran_plain = plain ? 1 : 0;
    // a launch on its own (not one of several frames in flight): persistent waves at full
    // occupancy balance the tiles dynamically, where a fixed tiles-per-wave grid makes every
    // wave render exactly that many tiles and the slowest wave's sum the makespan
    // (2: launches below RG_LIGHT_BIG_TILES tiles only -- rg_render_multi's shares and bands)
    if constexpr (SPARSE) {  // MAXD == 0: one instantiation per light-batch width
#if RG_LB_ONE
        if (a->n_lights <= 1) return launch_waves<0, RG_LIGHT_WPS_ONE, -1, false, false, false, 0, false, true>(a, stream, gt);
#endif
#if RG_LB_SMALL > 1
        if (a->n_lights <= RG_LB_SMALL) return launch_waves<0, RG_LIGHT_WPS, RG_LB_SMALL, false, false, false, 0, false, true>(a, stream, gt);
#endif
        return launch_waves<0, RG_LIGHT_WPS, RG_LB, false, false, false, 0, false, true>(a, stream, gt);
    } else {
    const bool persistent = MAXD != 0 && RG_LIGHT_SINGLE_PERSISTENT && !a->pipelined &&
                            (RG_LIGHT_SINGLE_PERSISTENT != 2 || rg_tile_count(*a) < RG_LIGHT_BIG_TILES);
#if RG_LB_ONE
    // one-light scenes: a batch of one (template LBT -1: 1 is the heavy path)
    if (a->n_lights <= 1) {
        if constexpr (MAXD != 0 && RG_LIGHT_SINGLE_PERSISTENT)
            if (persistent) return launch_light_one<MAXD, RG_LIGHT_WPS_ONE, -1, -1>(a, stream, gt, plain);
        return launch_light_one<MAXD, RG_LIGHT_WPS_ONE, -1, 0>(a, stream, gt, plain);
    }
#endif
#if RG_LB_SMALL > 1
    // scenes with at most RG_LB_SMALL lights: a batch that wide, not RG_LB (the per-light
    // loops of the shadow batch are unrolled over LB; test3's one light: 0.2525 -> 0.2293 ms
    // at LB 2, profiles/r06/s24)
    if (a->n_lights <= RG_LB_SMALL) {
        if constexpr (MAXD != 0 && RG_LIGHT_SINGLE_PERSISTENT)
            if (persistent) return launch_light_one<MAXD, RG_LIGHT_WPS, RG_LB_SMALL, -1>(a, stream, gt, plain);
        return launch_light_one<MAXD, RG_LIGHT_WPS, RG_LB_SMALL, 0>(a, stream, gt, plain);
    }
#endif
    if constexpr (MAXD != 0 && RG_LIGHT_SINGLE_PERSISTENT)
        if (persistent) return launch_light_one<MAXD, RG_LIGHT_WPS, RG_LB, -1>(a, stream, gt, plain);
#if RG_LIGHT_TPW_BIG > 0
    // whole frames (frames in flight): RG_LIGHT_TPW_BIG tiles per wave, half the waves of
    // RG_LIGHT_TILES_PER_WAVE (as a compile-time variant: test1 0.2968 -> 0.2943 ms over 200
    // frames, profiles/r06/s43); smaller launches (the 1/N shares) keep 16
    if constexpr (MAXD != 0)
        if (rg_tile_count(*a) >= RG_LIGHT_BIG_TILES)
            return launch_light_one<MAXD, RG_LIGHT_WPS, RG_LB, RG_LIGHT_TPW_BIG>(a, stream, gt, plain);
#endif
    return launch_light_one<MAXD, RG_LIGHT_WPS, RG_LB, 0>(a, stream, gt, plain);
    }
}

template <int MAXD, bool HF = false, bool SPARSE = false>
__attribute__((visibility("hidden"))) hipError_t launch_heavy(const RgKernelArgs *a, hipStream_t stream, size_t *gt) {
    const unsigned long long tiles = SPARSE ? a->tile_limit : rg_tile_count(*a);
    // frames in flight (pipelined): the throughput-sized grid already keeps blocks long;
    // task splitting then costs more than it saves (1/8 share 0.400 -> 0.384 ms without:
    // profiles/r02/ab_task_split.txt); a single small launch keeps it (its latency)
    const bool tasks = RG_HEAVY_TASKS && tiles < RG_HEAVY_TASK_TILES && !a->pipelined;
    if (a->n_nodes > 0)
        return tasks ? launch_waves<MAXD, RG_HEAVY_WPS, 1, true, true, true, 0, HF, SPARSE>(a, stream, gt)
                     : launch_waves<MAXD, RG_HEAVY_WPS, 1, true, true, false, 0, HF, SPARSE>(a, stream, gt);
    return tasks ? launch_waves<MAXD, RG_HEAVY_WPS, 1, RG_HEAVY_F32_FILTER, false, true, 0, HF, SPARSE>(a, stream, gt)
                 : launch_waves<MAXD, RG_HEAVY_WPS, 1, RG_HEAVY_F32_FILTER, false, false, 0, HF, SPARSE>(a, stream, gt);
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
