// rg_k_trace.h — Scene::trace for primary and query rays, and the shadow batches.
#pragma once
#include <hip/hip_runtime.h>

#include "rg_bvh_ray.h"
#include "rg_device.h"
#include "rg_k_bvh.h"
#include "rg_k_intersect.h"
#include "rg_k_math.h"
#include "rg_shadow_vol_cell.h"

#pragma clang fp contract(off)

namespace rgk {

// NODB (all three trace functions): the caller knows the scene has no disks and no boxes
// (rg_render_kernel's PLAIN instantiations), so those sections are not compiled in.
template <bool F32F, bool BVH, bool NODB = false, class Src>
__device__ __forceinline__ void trace_primary(const RgKernelArgs &a, const Src &src, V3 d, Closest &c) {
    if constexpr (!BVH) sph_primary<F32F>(a, src, d, c);
    // the camera buffer's list bounds, loaded while the other bodies are tested
    [[maybe_unused]] LbRange cam{0u, 0u, false};
    if constexpr (BVH) {
        if (a.lb_cam >= 0) cam = lbuf_begin(a, src, a.lb_cam, d, 0.0, 0.0, 0.0);
    }
    for (int i = 0; i < a.n_pln; ++i) {
        RG_REGION(RGR_PRIM_PLANE);
        const RgPln p = src.getp(i);
        double den = (p.nx * d.x + p.ny * d.y) + p.nz * d.z;   // bodies.rs:137
        if (den > 1e-6) {
            RG_REGION(RGR_PRIM_PLANE_DIV);
            double dist = p.on / den;                           // v = o_p - 0 = o_p: v.n = o.n
            if (dist >= 0.0) closest_add(c, dist, rg_cptr(a.pln_id)[i]);
        }
    }
    [[maybe_unused]] const V3 o = v3(0.0, 0.0, 0.0);
    if constexpr (!NODB) {
    for (int i = 0; i < a.n_dsk; ++i) {
        RG_REGION(RGR_DISK);
        const RgDsk k = src.getd(i);
        double t;
        if (disk_hit(k, o, d, t)) closest_add(c, t, rg_cptr(a.dsk_id)[i]);
    }
    if (a.n_box > 0) {
        RG_REGION(RGR_BOX);
        V3 inv = v3(1.0 / d.x, 1.0 / d.y, 1.0 / d.z);           // ray.rs:24
        int sx = inv.x < 0.0, sy = inv.y < 0.0, sz = inv.z < 0.0;
        for (int i = 0; i < a.n_box; ++i) {
            RG_REGION(RGR_BOX);
            const RgBox b = src.getb(i);
            double t;
            if (aabb_hit(b, o, inv, sx, sy, sz, t)) closest_add(c, t, rg_cptr(a.box_id)[i]);
        }
    }
    }
    if constexpr (BVH) {  // spheres last: the other bodies' hits already bound the search
        const bool ok = !c.nan && rg_bvh_ray_ok(a.bvh_obound, 0.0, 0.0, 0.0, d.x, d.y, d.z);
        RG_STAT(8, RG_LANES(!ok));
        if (!ok) {
            [[maybe_unused]] const unsigned long long t0 = RG_CLOCK();
            sph_primary<F32F>(a, src, d, c);
            RG_STAT(13, RG_CLOCK() - t0);
        }
        const bool walk = ok && !cam.use;
        if (ok && cam.use) cambuf_primary(a, src, cam, d, (float)d.x, (float)d.y, (float)d.z, c);
        if (walk) {
            bool need = true, unused = false;
            bvh_spheres<0>(a, src, o, d, false, 0.0, 0.0, c, unused, need);
        }
    }
}

// General query: closest-hit for secondary rays, any-hit for shadow rays.
// A shadow ray is occluded iff some body has a hit distance t with
// !(t > light_distance)  <=>  !(min t > light_distance)  (rendering.rs:152-155),
// so a lane stops testing at its first such hit and the wave leaves the body
// loops as soon as every lane that is still testing is a finished shadow ray.
template <bool F32F, bool BVH, bool NODB = false, class Src>
__device__ __forceinline__ void trace_query(const RgKernelArgs &a, const Src &src, const Ray &r, bool shadow, double ld,
                                            Closest &c, bool &occl, bool lane_walk = false, int light = -1) {
    const V3 o = r.o, d = r.d;
    bool need = true;
    if constexpr (!BVH) {
        if (!sph_query<F32F>(a, src, o, d, shadow, ld, c, occl, need)) return;
    }
    // shadow rays of a light with a buffer: the ray's list bounds, loaded while the planes,
    // disks and boxes are tested
    [[maybe_unused]] LbRange lbr{0u, 0u, false};
    if constexpr (BVH) {
        if (shadow && light >= 0 && light < a.n_lbuf) {
            const V3 lp = lbuf_light_pos(src, light);
            lbr = lbuf_begin(a, src, light, o, lp.x, lp.y, lp.z);
        }
    }
    for (int i = 0; i < a.n_pln; ++i) {
        const RgPln p = src.getp(i);
        double den = (p.nx * d.x + p.ny * d.y) + p.nz * d.z;   // bodies.rs:137-148
        RG_REGION(RGR_QC_PLANE);
        if (den > 1e-6 && need) {
            double vx = p.ox - o.x, vy = p.oy - o.y, vz = p.oz - o.z;
            double dist = ((vx * p.nx + vy * p.ny) + vz * p.nz) / den;
            if (dist >= 0.0) {
                if (shadow) {
                    if (!(dist > ld)) { occl = true; need = false; }
                } else {
                    closest_add(c, dist, rg_cptr(a.pln_id)[i]);
                }
            }
        }
    }
    if constexpr (NODB && !BVH) return;  // the planes were the last bodies
    if (!__any(need)) return;
    if constexpr (!NODB) {
    for (int i = 0; i < a.n_dsk; ++i) {
        RG_REGION(RGR_DISK);
        const RgDsk k = src.getd(i);
        double t;
        if (need && disk_hit(k, o, d, t)) {
            if (shadow) {
                if (!(t > ld)) { occl = true; need = false; }
            } else {
                closest_add(c, t, rg_cptr(a.dsk_id)[i]);
            }
        }
    }
    if (a.n_box > 0 && __any(need)) {
        RG_REGION(RGR_BOX);
        V3 inv = v3(1.0 / d.x, 1.0 / d.y, 1.0 / d.z);
        int sx = inv.x < 0.0, sy = inv.y < 0.0, sz = inv.z < 0.0;
        for (int i = 0; i < a.n_box; ++i) {
            RG_REGION(RGR_BOX);
            const RgBox b = src.getb(i);
            double t;
            if (need && aabb_hit(b, o, inv, sx, sy, sz, t)) {
                if (shadow) {
                    if (!(t > ld)) { occl = true; need = false; }
                } else {
                    closest_add(c, t, rg_cptr(a.box_id)[i]);
                }
            }
        }
    }
    }
    if constexpr (BVH) {  // spheres last: plane/disk/box hits already bound the search
        if (!__any(need)) return;
        double t0s = 0.0;
        float grow = 0.0f;
        const int cls = (need && !c.nan) ? rg_bvh_classify(a.bvh_obound, a.bvh_rbound, a.bvh_margin, a.bvh_extent,
                                                           o.x, o.y, o.z, d.x, d.y, d.z, t0s, grow)
                                         : RG_BVH_SCAN;
        // shadow rays of a light with a light buffer: their cell's spheres instead of the walk (near rays)
        const bool lb = shadow && need && cls == RG_BVH_TRAVERSE && grow == 0.0f && lbr.use;
        if (lb) lbuf_shadow(a, src, light, lbr, o, d, ld, occl, need);
        const bool ok = need && cls == RG_BVH_TRAVERSE && !lb;
#ifdef RG_BVH_STATS
        {
            RG_STAT(8, RG_LANES(need && cls == RG_BVH_SCAN));
            RG_STAT(9, RG_LANES(need && cls == RG_BVH_TRAVERSE && grow > 0.0f));
            RG_STAT(10, RG_LANES(need && cls == RG_BVH_NO_SPHERE));
            RG_STAT(11, RG_LANES(need && c.nan));
        }
#endif
        if (need && cls == RG_BVH_SCAN) {
            [[maybe_unused]] const unsigned long long t0 = RG_CLOCK();
            bool nd = true;
            sph_query<F32F>(a, src, o, d, shadow, ld, c, occl, nd);
            RG_STAT(13, RG_CLOCK() - t0);
        }
        const bool grown = ok && grow > 0.0f;  // far rays: boxes grown in the slab test
        // one walk kind per wave: if any lane's ray is incoherent, every near lane walks per lane
        // (a mixed wave would otherwise run the per-lane walk and then the wave walk)
        const bool per_lane = ok && !grown && a.lane_stack > 0 && __any(ok && !grown && lane_walk);
        if (per_lane) bvh_lane(a, src, o, d, shadow, ld, t0s, c, occl, need);
        if (ok && !grown && !per_lane) {
            bvh_spheres<1>(a, src, o, d, shadow, ld, t0s, c, occl, need);
        }
        if (grown) {
            bvh_spheres<1, true>(a, src, o, d, shadow, ld, t0s, c, occl, need, grow);
        }
    }
}

// A query ray whose arithmetic may overflow.  With every scene coordinate
// below 1e100 in magnitude (the host's `nan_scene` test, rg_capi.hip), a ray
// with |o_k| < 1e100 and |d_k| < 1e50 keeps every intermediate of the body
// tests (bodies.rs:92-119, 136-148, 173-192, 242-282) finite, so no hit
// distance can be NaN and Scene::trace's `partial_cmp().unwrap()`
// (scene.rs:38) cannot panic.  Anything else (NaN/inf included: the
// comparisons are false) is exotic and takes the exact, fully counted query.
__device__ __forceinline__ bool ray_exotic(V3 o, V3 d) {
    const bool ok = fabs(o.x) < 1e100 && fabs(o.y) < 1e100 && fabs(o.z) < 1e100 && fabs(d.x) < 1e50 &&
                    fabs(d.y) < 1e50 && fabs(d.z) < 1e50;
    return !ok;
}

// ---------------------------------------------------------------- shadow batches
// shade_diffuse traces one shadow ray per light from the SAME origin
// hit + n*bias (rendering.rs:141-150).  A lane traces up to RG_LB of them in
// one pass: per sphere the origin-dependent part (h = c - o, h.h) is computed
// once and only adj/opp/compare are per light, so a 3-light batch costs
// 8 + 3*8 FP64 ops per sphere instead of 3*16, with bit-identical per-ray
// arithmetic.  Bit l of `occl` = light l of the batch is occluded.
// RG_LB (lights per shadow batch on the light path) lives in rg_device.h
#ifndef RG_SHADOW_GROUP
#define RG_SHADOW_GROUP 2  // spheres per miss-test group in the shadow pass
#endif
// (RG_PLAIN_SHVOL and its two parts, the PLAIN kernels' shadow mask volume: rg_device.h)

template <int LB>
struct ShadowBatch {
    V3 d[LB];           // direction_from(light) (lights.rs:46-51)
    double ld[LB];      // light.distance(hit) (lights.rs:53-58), +inf for directional
};

// OR of v over the 64 lanes of a wave whose lanes are all active, as a wave-uniform value: four row
// shifts and two row broadcasts (DPP; a lane without a source ORs in 0) leave it in lane 63.
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1, 3
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// One miss-test group of the shadow pass: spheres idx[0 .. g) (g <= RG_SHADOW_GROUP, wave-uniform)
// against the batch's lights; bit l of `occl` is set where sphere and light l occlude (a: the region counters).
template <int LB, class Src>
__device__ __forceinline__ void shadow_group([[maybe_unused]] const RgKernelArgs &a, const Src &src, V3 o, const ShadowBatch<LB> &sb,
                                             const int (&idx)[RG_SHADOW_GROUP], int g, uint32_t &occl) {
    constexpr int G = RG_SHADOW_GROUP;
    RG_REGION(RGR_SH_GROUP);
    RgSph s[G];
    double hx[G], hy[G], hz[G], hh[G], adj[G][LB], opp[G][LB];
    bool cand[G][LB];
    bool any = false;
#pragma unroll
    for (int k = 0; k < G; ++k) {
        if (k < g) {
            s[k] = src.get(idx[k]);
            hx[k] = s[k].cx - o.x; hy[k] = s[k].cy - o.y; hz[k] = s[k].cz - o.z;   // bodies.rs:92
            hh[k] = (hx[k] * hx[k] + hy[k] * hy[k]) + hz[k] * hz[k];                // :95 (first term)
#pragma unroll
            for (int l = 0; l < LB; ++l) {
                adj[k][l] = (hx[k] * sb.d[l].x + hy[k] * sb.d[l].y) + hz[k] * sb.d[l].z;   // :93
                opp[k][l] = hh[k] - adj[k][l] * adj[k][l];                               // :95
                cand[k][l] = !(opp[k][l] > s[k].r2) && !((occl >> l) & 1u);              // :99
                any |= cand[k][l];
            }
        }
    }
    if (any) {
        RG_REGION(RGR_SH_TAIL);
#pragma unroll
        for (int k = 0; k < G; ++k) {
#pragma unroll
            for (int l = 0; l < LB; ++l) {
                double t;
#ifdef RG_REGION_STATS
                if (k < g && cand[k][l]) RG_REGION(RGR_SH_PAIR);
#endif
                if (k < g && cand[k][l] && sphere_tail(s[k].r2, opp[k][l], adj[k][l], t) && !(t > sb.ld[l]))
                    occl |= 1u << l;
            }
        }
    }
}

// SHV (the PLAIN kernels with RG_PLAIN_SHVOL): the wave's shadow mask (rg_shadow_vol.h), wave-uniform
// -- bit i of `smask` clear: no lane's ray can be occluded by sphere i, bit j of `pmask`: by plane j
// (bodies past the masks' bits are always tested; all ones without a volume).  The walk takes its
// groups from the set bits.  `occl` is an OR of hits and a skipped body has none, so the result is the
// full scan's in any order.
template <int LB, bool NODB = false, bool SHV = false, class Src>
__device__ __forceinline__ void trace_shadow(const RgKernelArgs &a, const Src &src, V3 o, const ShadowBatch<LB> &sb,
                                             uint32_t full, uint32_t &occl, [[maybe_unused]] uint32_t smask = ~0u,
                                             [[maybe_unused]] uint32_t pmask = ~0u) {
    constexpr int G = RG_SHADOW_GROUP;
    const int n = a.n_sph;
    if constexpr (SHV && RG_PLAIN_SHVOL_SPHERES != 0) {
        for (int base = 0; base < n; base += 32) {  // 32 spheres per pass: the first pass's under the mask
            const uint32_t lim = n - base >= 32 ? ~0u : (1u << (n - base)) - 1u;
            uint32_t left = base == 0 ? smask & lim : lim;
            for (int ng = 1; left != 0u; ++ng) {
                int idx[G], g = 0;
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    idx[k] = 0;
                    if (left != 0u) {
                        idx[k] = base + __builtin_ctz(left);
                        left &= left - 1u;
                        g = k + 1;
                    }
                }
                shadow_group<LB>(a, src, o, sb, idx, g, occl);
                if ((ng & 3) == 0 && !__any(occl != full)) return;
            }
        }
    } else {
    // (shadow_group's body, kept as it stood: routed through the helper, the kernels without the
    // mask compiled to other code than their parent's -- profiles/shvol/kernel_isa_diff.txt)
    const int nfull = n - n % G;
    for (int i = 0; i < n;) {
        const int g = i < nfull ? G : 1;  // wave-uniform
        RG_REGION(RGR_SH_GROUP);
        RgSph s[G];
        double hx[G], hy[G], hz[G], hh[G], adj[G][LB], opp[G][LB];
        bool cand[G][LB];
        bool any = false;
#pragma unroll
        for (int k = 0; k < G; ++k) {
            if (k < g) {
                s[k] = src.get(i + k);
                hx[k] = s[k].cx - o.x; hy[k] = s[k].cy - o.y; hz[k] = s[k].cz - o.z;   // bodies.rs:92
                hh[k] = (hx[k] * hx[k] + hy[k] * hy[k]) + hz[k] * hz[k];                // :95 (first term)
#pragma unroll
                for (int l = 0; l < LB; ++l) {
                    adj[k][l] = (hx[k] * sb.d[l].x + hy[k] * sb.d[l].y) + hz[k] * sb.d[l].z;   // :93
                    opp[k][l] = hh[k] - adj[k][l] * adj[k][l];                               // :95
                    cand[k][l] = !(opp[k][l] > s[k].r2) && !((occl >> l) & 1u);              // :99
                    any |= cand[k][l];
                }
            }
        }
        if (any) {
            RG_REGION(RGR_SH_TAIL);
#pragma unroll
            for (int k = 0; k < G; ++k) {
#pragma unroll
                for (int l = 0; l < LB; ++l) {
                    double t;
#ifdef RG_REGION_STATS
                    if (k < g && cand[k][l]) RG_REGION(RGR_SH_PAIR);
#endif
                    if (k < g && cand[k][l] && sphere_tail(s[k].r2, opp[k][l], adj[k][l], t) && !(t > sb.ld[l]))
                        occl |= 1u << l;
                }
            }
        }
        i += g;
        if ((i & 7) == 0 && !__any(occl != full)) return;
    }
    }
    if (!__any(occl != full)) return;
    for (int i = 0; i < a.n_pln; ++i) {
        if constexpr (SHV && RG_PLAIN_SHVOL_PLANES != 0) {
            if (i < RG_SHVOL_MAX_BODIES && !((pmask >> i) & 1u)) continue;  // (wave-uniform)
        }
        const RgPln p = src.getp(i);
        const double vx = p.ox - o.x, vy = p.oy - o.y, vz = p.oz - o.z;     // bodies.rs:139
        const double num = (vx * p.nx + vy * p.ny) + vz * p.nz;             // :140 numerator
        RG_REGION(RGR_SH_PLANE);
#pragma unroll
        for (int l = 0; l < LB; ++l) {
            const double den = (p.nx * sb.d[l].x + p.ny * sb.d[l].y) + p.nz * sb.d[l].z;  // :137
            if (den > 1e-6 && !((occl >> l) & 1u)) {
                bool hit;
                if (sb.ld[l] == __builtin_inf() && num >= 0.0) {
                    hit = true;  // fl(num/den) >= 0 and !(fl(num/den) > inf): no division needed
                } else {
                    RG_REGION(RGR_SH_PLANE_DIV);
                    const double dist = num / den;
                    hit = dist >= 0.0 && !(dist > sb.ld[l]);
                }
                if (hit) occl |= 1u << l;
            }
        }
    }
    if constexpr (NODB) return;  // the planes were the last bodies
    if (!__any(occl != full)) return;
    for (int i = 0; i < a.n_dsk; ++i) {
        RG_REGION(RGR_DISK);
        const RgDsk k = src.getd(i);
#pragma unroll
        for (int l = 0; l < LB; ++l) {
            double t;
            if (!((occl >> l) & 1u) && disk_hit(k, o, sb.d[l], t) && !(t > sb.ld[l])) occl |= 1u << l;
        }
    }
    if (a.n_box > 0 && __any(occl != full)) {
        RG_REGION(RGR_BOX);
#pragma unroll
        for (int l = 0; l < LB; ++l) {
            const V3 d = sb.d[l];
            const V3 inv = v3(1.0 / d.x, 1.0 / d.y, 1.0 / d.z);
            const int sx = inv.x < 0.0, sy = inv.y < 0.0, sz = inv.z < 0.0;
            for (int i = 0; i < a.n_box; ++i) {
                RG_REGION(RGR_BOX);
                const RgBox b = src.getb(i);
                double t;
                if (!((occl >> l) & 1u) && aabb_hit(b, o, inv, sx, sy, sz, t) && !(t > sb.ld[l])) occl |= 1u << l;
            }
        }
    }
}

}  // namespace rgk
