// rg_k_bvh.h — BVH traversal (the wave walk and the per-lane walk), the light and camera buffers.
#pragma once
#include <hip/hip_runtime.h>

#include "rg_bvh_ray.h"
#include "rg_device.h"
#include "rg_k_intersect.h"
#include "rg_k_math.h"
#include "rg_lightbuf_ray.h"

#pragma clang fp contract(off)

namespace rgk {

// ---------------------------------------------------------------- BVH traversal
// (the tree is built on the host by rg_bvh.cpp.)  The wave
// walks ONE node at a time: every lane tests the node's child boxes against
// its own ray (f32 slab test, rg_bvh_ray.h), the wave ballots, a leaf hit by
// any lane is tested at once by the lanes whose box test passed (f32 sphere
// pre-filter, then the reference's f64 test), and the internal children hit by
// any lane are visited depth-first, nearest first by the first active lane's
// entry distance, through a wave-uniform stack in LDS (one 64-entry stack per
// wave, written by the first active lane).  Boxes only cull spheres the exact
// test would reject or whose hit cannot be <= the lane's current best (closest
// hit) or light distance (shadow), and closest_add is order-independent, so the
// result and every distance equal the brute-force scan.  Lanes whose ray is
// outside the boxes' error analysis (rg_bvh_ray_ok) or whose closest-hit query
// already saw a NaN distance (AABB; nhit must stay exact) use the brute-force
// loop instead.
#define RG_BVH_STACK 64
__shared__ int rg_bvh_stack[RG_BVH_MAX_WAVES][RG_BVH_STACK];  // allocated only by kernels that traverse

__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Diagnostic build (-DRG_BVH_STATS): counters[4..15] = traversals, node visits,
// leaf visits (per wave), lanes traversing, lanes scanning all spheres (any
// reason), ... by reason (origin out of bound, |d| not unit, NaN), wave clock
// cycles in traversals, in full scans, in the whole kernel, waves.
#ifdef RG_BVH_STATS
// accumulated per wave in LDS (cheap), flushed to counters[] once per wave
__shared__ unsigned long long rg_stat_lds[RG_BVH_MAX_WAVES][16];
#define RG_STAT(word, v)                                                                        \
    do {                                                                                        \
        const unsigned long long rg_stat_v = (unsigned long long)(v);                           \
        if ((threadIdx.x & 63u) == (unsigned)__builtin_amdgcn_readfirstlane(threadIdx.x & 63u)) \
            rg_stat_lds[(threadIdx.x >> 6) % RG_BVH_MAX_WAVES][word] += rg_stat_v;              \
    } while (0)
#define RG_LANES(pred) __builtin_popcountll(__ballot(pred))
#define RG_CLOCK() ((unsigned long long)wall_clock64())
#else
#define RG_STAT(word, v) do { } while (0)
#define RG_LANES(pred) 0
#define RG_CLOCK() 0ull
#endif
__device__ __forceinline__ float wave_uniform_f(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

template <class Src>
__device__ __forceinline__ void leaf_primary(const RgKernelArgs &a, const Src &src, int first, int count, V3 d,
                                             float dx, float dy, float dz, Closest &c) {
    for (int j = first; j < first + count; ++j) {
        const RgSphF2 f2 = src.getf2(j);
        if (filter_primary(src.getf(j), f2, dx, dy, dz)) {
            const RgSph s = src.get(j);
            const double cc = src.getcc(j);
            const double adj = (s.cx * d.x + s.cy * d.y) + s.cz * d.z;
            const double opp = cc - adj * adj;
            double t;
            if (!(opp > s.r2) && sphere_tail(s.r2, opp, adj, t)) closest_add(c, t, f2.id);
        }
    }
}

template <class Src>
__device__ __forceinline__ void leaf_query(const RgKernelArgs &a, const Src &src, int first, int count, V3 o, V3 d,
                                           const RayF &rf, bool shadow, double ld, Closest &c, bool &occl,
                                           bool &need) {
    for (int j = first; j < first + count; ++j) {
        // the id comes with the filter record (RgSphF2::id): a per-lane j (bvh_lane) would
        // otherwise make sph_id[j] a vector global load whose latency the hit waits for
        const RgSphF f = src.getf(j);
        const RgSphF2 f2 = src.getf2(j);
        if (need && filter_general(f, f2, rf)) {
            const RgSph s = src.get(j);
            const double hx = s.cx - o.x, hy = s.cy - o.y, hz = s.cz - o.z;
            const double adj = (hx * d.x + hy * d.y) + hz * d.z;
            const double opp = ((hx * hx + hy * hy) + hz * hz) - adj * adj;
            double t;
            if (!(opp > s.r2) && sphere_tail(s.r2, opp, adj, t)) {
                if (shadow) {
                    if (!(t > ld)) { occl = true; need = false; }
                } else {
                    closest_add(c, t, f2.id);
                }
            }
        }
    }
}

// KIND 0: primary ray (o = 0); 1: a query, per lane closest hit or (`shadow`)
// any hit with t <= ld -- closest-hit and shadow lanes of a wave share ONE walk
// instead of running one walk per kind one after the other.
// Called by the lanes that take the BVH (exec mask); `need` drops for a
// shadow lane at its first occluder.  The box tests start at o + t0s d
// (t0s > 0 only for far origins, rg_bvh_classify) and prune against
// distances shifted by t0s; the exact sphere tests use the ray as given.
__device__ __forceinline__ float bvh_bound(double v) { return v <= 0.0 ? 0.0f : rg_f32_up(v); }

template <int KIND, bool GROW = false, class Src>
__device__ __forceinline__ void bvh_spheres(const RgKernelArgs &a, const Src &src, V3 o, V3 d, bool shadow, double ld,
                                            double t0s, Closest &c, bool &occl, bool &need, float grow = 0.0f) {
    int *stack = rg_bvh_stack[threadIdx.x >> 6];
    const V3 ob = t0s > 0.0 ? add(o, scl(d, t0s)) : o;
    const RayB rb = rg_make_rayb(ob.x, ob.y, ob.z, d.x, d.y, d.z);
    RayF rf;
    const float dx = (float)d.x, dy = (float)d.y, dz = (float)d.z;
    if constexpr (KIND != 0) rf = make_rayf(o, d);
    const float tld = shadow ? bvh_bound(ld - t0s) : 0.0f;
    const int lane = (int)(threadIdx.x & 63u);
    const bool writer = lane == wave_uniform(lane);
    int sp = 0;
    int node = 0;
    RG_STAT(4, 1);
    RG_STAT(7, RG_LANES(1));
    [[maybe_unused]] const unsigned long long t_in = RG_CLOCK();
    for (;;) {
        RG_STAT(5, 1);
        const RgBvhNode N = src.getn_uniform(node);
        const int nch = wave_uniform(N.nchild);
        const float tb = shadow ? tld : (c.id >= 0 ? bvh_bound(c.t - t0s) : __builtin_huge_valf());
        int next = -1;
        float next_key = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < nch) {
                float tn = 0.0f;
                const bool h = need && rg_child_hit<GROW>(N, k, rb, tb, tn, grow);
                if (__any(h)) {
                    const int ch = wave_uniform(N.child[k]);
                    if (ch < 0) {
                        const int v = ~ch, first = v >> 3, count = (v & 7) + 1;
                        RG_STAT(6, 1);
                        if (h) {
                            if constexpr (KIND == 0) leaf_primary(a, src, first, count, d, dx, dy, dz, c);
                            else leaf_query(a, src, first, count, o, d, rf, shadow, ld, c, occl, need);
                        }
                    } else {
                        const float key = wave_uniform_f(h ? tn : __builtin_huge_valf());
                        int push = ch;
                        if (next < 0 || key < next_key) {
                            push = next;
                            next = ch;
                            next_key = key;
                        }
                        if (push >= 0 && sp < RG_BVH_STACK) {
                            if (writer) stack[sp] = push;
                            ++sp;
                        }
                    }
                }
            }
        }
        if constexpr (KIND != 0) {
            if (!__any(need)) break;  // every shadow lane occluded (closest-hit lanes keep `need`)
        }
        if (next >= 0) {
            node = next;
        } else {
            if (sp == 0) break;
            --sp;
            node = wave_uniform(stack[sp]);
        }
    }
    RG_STAT(12, RG_CLOCK() - t_in);
}

// Per-lane traversal for incoherent rays (secondary rays and the shadow rays
// of their hits).  The wave-coherent walk above visits the UNION of its lanes'
// paths; for 64 rays in 64 directions that is most of the tree, so every lane
// here walks its own path: nearest-first over the same 4-wide nodes (per-lane
// LDS gathers), the other hit children on a per-lane stack in LDS
// (RG_LANE_NODE_BITS entry format, rg_device.h), each popped entry skipped when
// its stored entry distance -- a lower bound -- already exceeds the current
// bound, exactly as a fresh slab test against that bound would skip it.  Same
// boxes, bounds and leaf tests (f32 pre-filter, then the exact f64 test) as
// bvh_spheres, so the accepted set and every distance are identical.  The host
// sizes the stack to the tree's worst case (rg_bvh.cpp lane_stack_need).
extern __shared__ __attribute__((aligned(16))) unsigned char rg_dyn_smem[];

__device__ __forceinline__ uint32_t lane_key(float tn, int node) {
    return (__float_as_uint(tn) & ~((1u << RG_LANE_NODE_BITS) - 1u)) | (uint32_t)node;
}
__device__ __forceinline__ float lane_key_t(uint32_t e) {
    return __uint_as_float(e & ~((1u << RG_LANE_NODE_BITS) - 1u));
}
__device__ __forceinline__ void cswap(uint32_t &x, uint32_t &y) {
    const uint32_t lo = min(x, y), hi = max(x, y);
    x = lo;
    y = hi;
}

template <class Src>
__device__ __forceinline__ void bvh_lane(const RgKernelArgs &a, const Src &src, V3 o, V3 d, bool shadow, double ld,
                                         double t0s, Closest &c, bool &occl, bool &need) {
    uint32_t *stk = reinterpret_cast<uint32_t *>(rg_dyn_smem) + threadIdx.x;  // entry e at stk[e * blockDim.x]
    const uint32_t stride = blockDim.x;
    const uint32_t mask = (1u << RG_LANE_NODE_BITS) - 1u;
    const V3 ob = t0s > 0.0 ? add(o, scl(d, t0s)) : o;
    const RayB rb = rg_make_rayb(ob.x, ob.y, ob.z, d.x, d.y, d.z);
    const RayF rf = make_rayf(o, d);
    const float tld = shadow ? bvh_bound(ld - t0s) : 0.0f;
    int node = 0;
    RG_STAT(4, 1);
    RG_STAT(7, RG_LANES(1));
    [[maybe_unused]] const unsigned long long t_in = RG_CLOCK();
    // slot `cap` is a spare: a write that is not a push may land there, never on an entry;
    // the stack pointer is kept scaled by the stride (spo = sp * stride: no multiplies)
    const uint32_t capo = (uint32_t)a.lane_stack * stride;
    uint32_t spo = 0u;
    for (;;) {
        const bool act = need && node >= 0;
        if (!__any(act)) break;
        RG_STAT(5, 1);
#ifdef RG_ITER_STATS  // per-lane walk: iterations, active lanes (counters[12..13])
        {
            const unsigned long long m = __ballot(act);
            if ((int)(threadIdx.x & 63u) == __builtin_ffsll((long long)__ballot(1)) - 1) {
                atomicAdd(&a.counters[12], 1ull);
                atomicAdd(&a.counters[13], (unsigned long long)__builtin_popcountll(m));
            }
        }
#endif
        if (act) {
            RG_REGION(RGR_WALK);  // per-lane walk iteration (heavy path)
            // the node's children without divergent branches: every slot's slab test,
            // hit leaves as a bit mask (tested below in child order), hit internal
            // children as sort keys (~0: none), pushes written unconditionally
            const RgBvhNode N = src.getn(node);
            const float tb = shadow ? tld : (c.id >= 0 ? bvh_bound(c.t - t0s) : __builtin_huge_valf());
            uint32_t e[4], leaves = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float tn = 0.0f;
                const bool h = (k < N.nchild) & rg_child_hit(N, k, rb, tb, tn);
                const int ch = N.child[k];
                leaves |= (h & (ch < 0)) ? (1u << k) : 0u;
                e[k] = (h & (ch >= 0)) ? lane_key(tn, ch) : ~0u;
            }
            // leaves first (they tighten a closest-hit bound), in child order
            while (leaves != 0u && need) {
                RG_REGION(RGR_WALK_LEAF);
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                const int v = ~(k == 0u ? N.child[0] : k == 1u ? N.child[1] : k == 2u ? N.child[2] : N.child[3]);
                leaf_query(a, src, v >> 3, (v & 7) + 1, o, d, rf, shadow, ld, c, occl, need);
            }
            uint32_t e0 = e[0], e1 = e[1], e2 = e[2], e3 = e[3];
            // ascending (entry distance, node); empty slots (~0) last
            cswap(e0, e1); cswap(e2, e3); cswap(e0, e2); cswap(e1, e3); cswap(e1, e2);
            stk[min(spo, capo)] = e3;
            spo += ((e3 != ~0u) & (spo < capo)) ? stride : 0u;
            stk[min(spo, capo)] = e2;
            spo += ((e2 != ~0u) & (spo < capo)) ? stride : 0u;
            stk[min(spo, capo)] = e1;
            spo += ((e1 != ~0u) & (spo < capo)) ? stride : 0u;
            const float tbn = shadow ? tld : (c.id >= 0 ? bvh_bound(c.t - t0s) : __builtin_huge_valf());
            if (e0 != ~0u && (shadow || !(lane_key_t(e0) > tbn))) {
                node = (int)(e0 & mask);
            } else {
                node = -1;
                while (spo > 0u && need) {
                    spo -= stride;
                    const uint32_t e = stk[spo];
                    if (shadow || !(lane_key_t(e) > tbn)) {
                        node = (int)(e & mask);
                        break;
                    }
                }
            }
        }
    }
    RG_STAT(13, RG_CLOCK() - t_in);  // per-lane walk: word 13 (with the rare full scans)
}

// Light buffers (rg_lightbuf_ray.h, rg_lightbuf.cpp) in two steps, so the list bounds' load is in
// flight while the plane/disk/box tests run: lbuf_begin finds the ray's cell and loads its list
// bounds, lbuf_finish tests the list's spheres (and the always list), each with the leaf tests' f32
// pre-filter and exact test.  The lists hold every sphere the exact test could accept for the ray,
// so the answer is the BVH walk's; use == false: the buffer does not cover this ray (origin beyond
// the near-ray bound, no direction) and the caller walks the BVH.
struct LbRange {
    uint32_t k0, k1;  // the cell's entries (k0 == k1: an empty cell)
    bool use;
};
template <class Src>
__device__ __forceinline__ LbRange lbuf_begin(const RgKernelArgs &a, const Src &src, int buf, V3 o, double lx,
                                              double ly, double lz) {
    LbRange r{0u, 0u, false};
    const RgLightBufDev &B = src.lb[buf];
    if (B.kind == RG_LB_NONE) return r;
    const int cell = rg_lb_cell(B, lx, ly, lz, o.x, o.y, o.z, a.bvh_obound);
    if (cell == RG_LB_SKIP) return r;
    r.use = true;
    if (cell >= 0) {
        const uint32_t *st = a.lb_start + B.cell_off + (uint32_t)cell;
        r.k0 = st[0];
        r.k1 = st[1];
    }
    return r;
}
// the light's position for a spherical light's buffer (directional: unused)
template <class Src>
__device__ __forceinline__ V3 lbuf_light_pos(const Src &src, int light) {
    const RgLightDev &L = src.lt[light];
    return v3(L.v[0], L.v[1], L.v[2]);
}

// Shadow ray of `light`: any hit with t <= ld among the listed spheres
template <class Src>
__device__ __forceinline__ void lbuf_shadow(const RgKernelArgs &a, const Src &src, int light, const LbRange &r, V3 o,
                                            V3 d, double ld, bool &occl, bool &need) {
    const RgLightBufDev &B = src.lb[light];
    RG_REGION(RGR_LB_SHADOW);
    const RayF rf = make_rayf(o, d);
    Closest unused;
    closest_init(unused);
    for (uint32_t k = B.always0; k < B.always1 && need; ++k)
        leaf_query(a, src, (int)a.lb_ent[k], 1, o, d, rf, true, ld, unused, occl, need);
    // the list's entries four at a time: their loads in flight together, not one round trip per sphere
    for (uint32_t k = r.k0; k < r.k1 && need; k += 4) {
        uint32_t j[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) j[i] = a.lb_ent[min(k + (uint32_t)i, r.k1 - 1u)];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (k + (uint32_t)i < r.k1 && need) leaf_query(a, src, (int)j[i], 1, o, d, rf, true, ld, unused, occl, need);
    }
}

// Primary ray through the camera buffer (a light buffer around the camera at the origin, ray.rs:53:
// every primary ray starts there; closest hit, order-independent rule)
template <class Src>
__device__ __forceinline__ void cambuf_primary(const RgKernelArgs &a, const Src &src, const LbRange &r, V3 d, float dx,
                                               float dy, float dz, Closest &c) {
    const RgLightBufDev &B = src.lb[a.lb_cam];
    for (uint32_t k = B.always0; k < B.always1; ++k) leaf_primary(a, src, (int)a.lb_ent[k], 1, d, dx, dy, dz, c);
    for (uint32_t k = r.k0; k < r.k1; k += 4) {
        uint32_t j[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) j[i] = a.lb_ent[min(k + (uint32_t)i, r.k1 - 1u)];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (k + (uint32_t)i < r.k1) leaf_primary(a, src, (int)j[i], 1, d, dx, dy, dz, c);
    }
}

}  // namespace rgk
