// rg_render_grid.h — how many blocks a launch of rg_render_kernel<K> gets: the arithmetic between
// the occupancy query and the launch (rg_render_launch.h launch_one).  Plain integer arithmetic
// over the configuration's facts (rg_render_cfg.h), no HIP: tests/native/render_cfg_test.cpp
// checks it on the CPU.
#pragma once
#include <algorithm>

#include "rg_render_cfg.h"

#ifndef RG_LIGHT_PERSIST_BLOCKS_PER_CU
// light persistent launches: one-wave blocks per CU (8 -> 6 once they stopped prefetching tile slots:
// test1 slowest 1/8 share 0.162-0.166 -> 0.153-0.156 ms, test3 0.139 -> 0.133; 4: 0.159, 12/16: slower;
// profiles/r05/s34, s35)
#define RG_LIGHT_PERSIST_BLOCKS_PER_CU 6
#endif
#ifndef RG_DEEP_BLOCKS_PER_CU
#define RG_DEEP_BLOCKS_PER_CU 8  // deep-stack light launches: resident one-wave blocks per CU (bounds the frame buffer)
#endif
#ifndef RG_PIPE_TILES_PER_WAVE
#define RG_PIPE_TILES_PER_WAVE 64  // heavy launches with frames in flight (RgKernelArgs::pipelined;
                                   // 32 -> 64: configs[4] scene at 1080p 2.50 -> 2.33 ms, profiles/r05/s21)
#endif
#ifndef RG_PIPE_MIN_CU_DIV
#define RG_PIPE_MIN_CU_DIV 4  // ... and at least 1/this of the CUs' blocks (3 -> 4: north-star 1/8 share 0.349 -> 0.327 ms)
#endif

// Blocks of the grid.  tiles: what the launch renders (a sparse launch: its list's length); cus and
// per_cu: the occupancy query's answer; pipelined: one of several frames in flight;
// max_grid_threads: nonzero = the cap the deep frame buffer's size puts on the grid.
// Persistent kernels: one block per CU slot, grid = CUs x (blocks per CU the register and LDS
// budgets admit), capped by the tiles the launch has.
template <class K>
constexpr unsigned long long rg_render_grid_blocks(unsigned long long tiles, int cus, int per_cu, bool pipelined,
                                                   unsigned long long max_grid_threads) {
    if (K::host_frames && K::light && per_cu > RG_DEEP_BLOCKS_PER_CU) per_cu = RG_DEEP_BLOCKS_PER_CU;
    // light single launches, persistent waves: RG_LIGHT_PERSIST_BLOCKS_PER_CU one-wave blocks per
    // CU (2 per SIMD), never more than the occupancy query admits (a scene whose LDS copy allows
    // fewer would otherwise start the extra blocks only after the queue drained)
    if (K::light_persistent) per_cu = std::min(per_cu, RG_LIGHT_PERSIST_BLOCKS_PER_CU);
    const unsigned long long waves = K::waves_per_block;
    unsigned long long blocks = (unsigned long long)cus * per_cu;
    const unsigned long long need = (tiles + waves - 1) / waves;
    if (blocks > need) blocks = need;
    if (!K::light && !K::global_frames && pipelined) {
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
    if constexpr (!K::persistent)  // one wave per K::tiles_per_wave tiles
        blocks = (tiles + waves * K::tiles_per_wave - 1) / (waves * K::tiles_per_wave);
    if (max_grid_threads && blocks * K::block_threads > max_grid_threads) blocks = max_grid_threads / K::block_threads;
    return blocks < 1 ? 1 : blocks;
}
