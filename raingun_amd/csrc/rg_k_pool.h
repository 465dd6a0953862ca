// rg_k_pool.h — the block-local task pool in LDS (task splitting on the heavy path).
#pragma once
#include <hip/hip_runtime.h>

#include "rg_k_math.h"

#pragma clang fp contract(off)

namespace rgk {

// ---------------------------------------------------------------- task splitting
// A refractive hit opens two independent subtrees (transmission, then
// reflection: rendering.rs:100-113); the lane traces the transmission ray and
// PUBLISHES the reflection ray in a block-local pool in LDS.  Any idle lane of
// the block (its pixel finished, or its wave out of tiles) may take it, trace
// the subtree with the same state machine and hand the colour back; if nobody
// took it by the time the owner needs it, the owner reclaims it and traces it
// itself.  A subtree's colour is a function of its ray only (in the area
// family, rg_area.h: of its ray and its owner's pixel, which pix carries to
// whoever traces it), and the owner
// combines it with exactly the expression of FR_REFR_R, so results are
// identical whoever traces it.  This splits the long ray trees of
// refractive pixels (the slowest tiles, which bound a frame's makespan)
// across the waves of a CU.  Waits only ever point down a tree, so there is
// no cycle: every awaited subtree is held by a live lane.
#ifndef RG_TASK_SLOTS
#define RG_TASK_SLOTS 128
#endif
struct TaskPool {
    static constexpr int S = RG_TASK_SLOTS;
    static_assert(S % 32 == 0, "whole bitmap words");
    double ray[S][6];  // published ray (origin, direction)
    float col[S][4];   // the subtree's colour once done
    int depth[S];      // recursion depth of the published ray
    uint32_t pix[S];   // owner's pixel (error reports; the area family's light positions)
    int done[S];       // 1: col holds the result
    uint32_t free_m[S / 32];  // 1 = slot free
    uint32_t pend_m[S / 32];  // 1 = published, not taken
    int busy;                 // waves of the block that hold work
};
// one pool per block (heavy path: a CU's 12 waves); allocated only by the kernels that split tasks
__shared__ TaskPool rg_pool;
__device__ __forceinline__ TaskPool &pool_of() { return rg_pool; }
constexpr int pool_slots() { return RG_TASK_SLOTS; }

#define RG_WG __HIP_MEMORY_SCOPE_WORKGROUP
__device__ __forceinline__ void pool_init() {
    auto &P = pool_of();
    constexpr int S = pool_slots();
    if (threadIdx.x < S / 32) {
        P.free_m[threadIdx.x] = ~0u;
        P.pend_m[threadIdx.x] = 0u;
    }
    for (uint32_t k = threadIdx.x; k < (uint32_t)S; k += blockDim.x) P.done[k] = 0;
    if (threadIdx.x == 0) P.busy = 0;
}
// Claim a free slot (-1: pool full).  Lanes start at different words/bits.
__device__ __forceinline__ int pool_alloc(int lane) {
    auto &P = pool_of();
    constexpr int S = pool_slots();
    const int rot = (lane >> 2) & 31;
    for (int i = 0; i < S / 32; ++i) {
        const int w = (lane + i) & (S / 32 - 1);
        uint32_t m = __hip_atomic_load(&P.free_m[w], __ATOMIC_RELAXED, RG_WG);
        while (m != 0u) {
            const uint32_t r = rot ? ((m >> rot) | (m << (32 - rot))) : m;
            const int b = (__builtin_ctz(r) + rot) & 31;
            const uint32_t bit = 1u << b;
            const uint32_t old = __hip_atomic_fetch_and(&P.free_m[w], ~bit, __ATOMIC_ACQUIRE, RG_WG);
            if (old & bit) return w * 32 + b;
            m = old & ~bit;
        }
    }
    return -1;
}
__device__ __forceinline__ void pool_publish(int slot) {  // ray/depth/pix written before
    __hip_atomic_fetch_or(&pool_of().pend_m[slot >> 5], 1u << (slot & 31), __ATOMIC_RELEASE, RG_WG);
}
__device__ __forceinline__ bool pool_any_pending() {
    uint32_t m = 0u;
#pragma unroll
    for (int w = 0; w < pool_slots() / 32; ++w) m |= __hip_atomic_load(&pool_of().pend_m[w], __ATOMIC_RELAXED, RG_WG);
    return m != 0u;
}
// Take the k-th pending task of a snapshot (k = rank among the wave's idle lanes).
__device__ __forceinline__ int pool_take(int k) {
    auto &P = pool_of();
    for (int w = 0; w < pool_slots() / 32; ++w) {
        uint32_t m = __hip_atomic_load(&P.pend_m[w], __ATOMIC_RELAXED, RG_WG);
        const int n = __builtin_popcount(m);
        if (k >= n) {
            k -= n;
            continue;
        }
        for (int j = 0; j < k; ++j) m &= m - 1u;
        const uint32_t bit = m & (~m + 1u);
        const uint32_t old = __hip_atomic_fetch_and(&P.pend_m[w], ~bit, __ATOMIC_ACQUIRE, RG_WG);
        return (old & bit) ? w * 32 + __builtin_ctz(bit) : -1;
    }
    return -1;
}
__device__ __forceinline__ bool pool_reclaim(int slot) {  // owner: un-publish if still pending
    const uint32_t bit = 1u << (slot & 31);
    return (__hip_atomic_fetch_and(&pool_of().pend_m[slot >> 5], ~bit, __ATOMIC_ACQ_REL, RG_WG) & bit) != 0u;
}
__device__ __forceinline__ void pool_finish(int slot, C3 c) {  // taker: result, then done
    auto &P = pool_of();
    P.col[slot][0] = c.r;
    P.col[slot][1] = c.g;
    P.col[slot][2] = c.b;
    __hip_atomic_store(&P.done[slot], 1, __ATOMIC_RELEASE, RG_WG);
}
__device__ __forceinline__ bool pool_done(int slot) {
    return __hip_atomic_load(&pool_of().done[slot], __ATOMIC_ACQUIRE, RG_WG) != 0;
}
__device__ __forceinline__ void pool_release(int slot) {  // owner: slot free again
    auto &P = pool_of();
    __hip_atomic_store(&P.done[slot], 0, __ATOMIC_RELAXED, RG_WG);
    __hip_atomic_fetch_or(&P.free_m[slot >> 5], 1u << (slot & 31), __ATOMIC_RELEASE, RG_WG);
}

}  // namespace rgk
