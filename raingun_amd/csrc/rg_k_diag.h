// rg_k_diag.h — what the render kernel's diagnostic builds run that needs no state of the kernel's
// own: the SIMD-use counters of -DRG_ITER_STATS (scripts/iter_stats.py), and whether a.rgb is the
// f32 output at all.  The library's build compiles none of it.  The timelines (-DRG_TILE_TIMES,
// -DRG_WAVE_TIMES) stay in rg_render_kernel, variables and code: behind functions -- members of a
// struct holding their state, a function taking the values, a local lambda -- those builds' kernels
// came out of the register allocator a VGPR or a scratch slot apart (profiles/cfg/README.md), and
// an instrument should measure the kernel it was calibrated on.  (RG_BVH_STATS: rg_k_bvh.h;
// RG_REGION_STATS: rg_k_math.h.)
#pragma once
#include <hip/hip_runtime.h>

#include "rg_device.h"
#include "rg_k_math.h"

namespace rgk {

struct KDiag {
    // The timelines (RG_TILE_TIMES, RG_WAVE_TIMES) go out through a.rgb, so those builds store no f32 RGB there.
#if defined(RG_TILE_TIMES) || defined(RG_WAVE_TIMES)
    static constexpr bool rgb_is_output = false;
#else
    static constexpr bool rgb_is_output = true;
#endif

    // SIMD use of the query iterations (RG_ITER_STATS), counters[4..11]: query iterations, their
    // querying lanes; iterations with a ray of depth >= 1, their querying lanes, their depth >= 1
    // lanes; iterations with <= 16 querying lanes; iterations with shadow lanes, shadow lanes.
    // depth: the lane's ray's.  Nothing in the other builds.
    template <bool LIGHT>
    static __device__ __forceinline__ void iter_stats([[maybe_unused]] const RgKernelArgs &a, [[maybe_unused]] int lane,
                                                      [[maybe_unused]] bool querying, [[maybe_unused]] int mode,
                                                      [[maybe_unused]] int depth) {
#ifdef RG_ITER_STATS
        const unsigned long long all = __ballot(querying), sec = __ballot(querying && depth >= 1);
        const unsigned long long shl = __ballot(querying && mode != MODE_CLOSEST);
        const unsigned n = (unsigned)__builtin_popcountll(all);
        if (lane == __builtin_ffsll((long long)__ballot(1)) - 1) {  // one atomic set per wave iteration
            atomicAdd(&a.counters[4], 1ull);
            atomicAdd(&a.counters[5], (unsigned long long)n);
            if (sec) {
                atomicAdd(&a.counters[6], 1ull);
                atomicAdd(&a.counters[7], (unsigned long long)n);
                atomicAdd(&a.counters[8], (unsigned long long)__builtin_popcountll(sec));
            }
            if (n <= 16) atomicAdd(&a.counters[9], 1ull);
            if (shl) {
                atomicAdd(&a.counters[10], 1ull);
                atomicAdd(&a.counters[11], (unsigned long long)__builtin_popcountll(shl));
            }
            // light path (no BVH walk words): iterations with closest-hit lanes, those lanes
            if (LIGHT && (all & ~shl)) {
                atomicAdd(&a.counters[14], 1ull);
                atomicAdd(&a.counters[15], (unsigned long long)__builtin_popcountll(all & ~shl));
            }
        }
#endif
    }
};

}  // namespace rgk
