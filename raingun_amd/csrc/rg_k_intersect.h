// rg_k_intersect.h — closest-hit records, the primitive tests, the sphere sources and the f32 pre-filter.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "rg_device.h"
#include "rg_k_math.h"

#pragma clang fp contract(off)

namespace rgk {

// ---------------------------------------------------------------- closest hit
// Scene::trace (scene.rs:34-39): first minimum in list order.  The body tables
// are grouped by kind, so ties across groups are broken by the YAML index.
struct Closest {
    double t;
    int id;
    int nhit;
    bool nan;
};
__device__ __forceinline__ void closest_init(Closest &c) { c.t = 0.0; c.id = -1; c.nhit = 0; c.nan = false; }
__device__ __forceinline__ void closest_add(Closest &c, double t, int id) {
    c.nhit++;
    if (t != t) c.nan = true;
    if (c.id < 0 || t < c.t || (t == c.t && id < c.id)) { c.t = t; c.id = id; }
}

// Sphere tail after the opp <= r2 test (bodies.rs:105-119).
__device__ __forceinline__ bool sphere_tail(double r2, double opp, double adj, double &t) {
    double th = sqrt(r2 - opp);
    double d0 = adj - th, d1 = adj + th;
    if (d0 < 0.0 && d1 < 0.0) return false;
    t = d0 < 0.0 ? d1 : (d1 < 0.0 ? d0 : fmin(d0, d1));
    return true;
}

struct Ray {
    V3 o, d;
};

// AABB slab test (bodies.rs:242-282).  inv = 1/d, sg = (inv < 0).
__device__ __forceinline__ bool aabb_hit(const RgBox &b, V3 o, V3 inv, int sx, int sy, int sz, double &t) {
    double tmin = ((sx ? b.hi[0] : b.lo[0]) - o.x) * inv.x;
    double tmax = ((sx ? b.lo[0] : b.hi[0]) - o.x) * inv.x;
    double tymin = ((sy ? b.hi[1] : b.lo[1]) - o.y) * inv.y;
    double tymax = ((sy ? b.lo[1] : b.hi[1]) - o.y) * inv.y;
    if (tmin > tymax || tymin > tmax) return false;
    if (tymin > tmin) tmin = tymin;
    if (tymax < tmax) tmax = tymax;
    double tzmin = ((sz ? b.hi[2] : b.lo[2]) - o.z) * inv.z;
    double tzmax = ((sz ? b.lo[2] : b.hi[2]) - o.z) * inv.z;
    if (tmin > tzmax || tzmin > tmax) return false;
    if (tzmin > tmin) tmin = tzmin;
    if (tzmax < tmax) tmax = tzmax;
    if (tmin >= 0.0) { t = tmin; return true; }
    if (tmax >= 0.0) { t = tmax; return true; }
    return false;
}

// Disk (bodies.rs:173-192).
__device__ __forceinline__ bool disk_hit(const RgDsk &k, V3 o, V3 d, double &t) {
    double den = (k.nx * d.x + k.ny * d.y) + k.nz * d.z;
    if (!(den > 1e-6)) return false;
    V3 v = v3(k.ox - o.x, k.oy - o.y, k.oz - o.z);
    double dist = ((v.x * k.nx + v.y * k.ny) + v.z * k.nz) / den;
    if (!(dist >= 0.0)) return false;
    V3 h = add(o, scl(d, dist));
    V3 w = v3(h.x - k.ox, h.y - k.oy, h.z - k.oz);
    if (!(sqrt(dot(w, w)) < k.r)) return false;
    t = dist;
    return true;
}

// ---------------------------------------------------------------- sphere sources
// The sphere tables are read with a wave-uniform index.  Three sources:
//  * SphLds: the persistent block stages the tables into LDS once and every
//    test reads them with broadcast ds_read_b128 (always a hit);
//  * SphScalar: scalar loads through the constant address space (s_load,
//    SGPR operands) for scenes whose tables exceed the LDS budget;
//  * SphNodesLds: the same, but the BVH nodes (read per lane by the per-lane
//    walk: vector loads from global memory otherwise) staged in LDS when the
//    sphere tables do not fit and the nodes do (BASELINE configs[4]: 4,096 spheres).
template <bool NODES_LDS>
struct SphGlobal {
    static constexpr bool in_lds = false;
    const RG_CONST RgSph *s;
    const RG_CONST double *cc;
    const RG_CONST RgSphF *f;
    const RG_CONST RgSphF2 *f2;
    const RG_CONST RgPln *pl;
    const RG_CONST RgDsk *dk;
    const RG_CONST RgBox *bx;
    typename std::conditional<NODES_LDS, const RgBvhNode *, const RG_CONST RgBvhNode *>::type nd;
    const RgLightBufDev *lb = nullptr;  // light-buffer descriptors (global)
    const RgLightDev *lt = nullptr;     // lights (global)
    __device__ __forceinline__ RgBvhNode getn(int i) const { return nd[i]; }
    __device__ __forceinline__ RgBvhNode getn_uniform(int i) const { return nd[i]; }
    __device__ __forceinline__ RgSph getv(int i) const { return ((const RgSph *)s)[i]; }
    __device__ __forceinline__ RgPln getp(int i) const { return pl[i]; }
    __device__ __forceinline__ RgDsk getd(int i) const { return dk[i]; }
    __device__ __forceinline__ RgBox getb(int i) const { return bx[i]; }
    __device__ __forceinline__ RgSph get(int i) const { return s[i]; }
    __device__ __forceinline__ double getcc(int i) const { return cc[i]; }
    __device__ __forceinline__ RgSphF getf(int i) const { return f[i]; }
    __device__ __forceinline__ RgSphF2 getf2(int i) const { return f2[i]; }
};
using SphScalar = SphGlobal<false>;
using SphNodesLds = SphGlobal<true>;
struct SphLds {
    static constexpr bool in_lds = true;
    const RgSph *s;
    const double *cc;
    const RgSphF *f;
    const RgSphF2 *f2;
    const RgPln *pl;
    const RgDsk *dk;
    const RgBox *bx;
    const RgBvhNode *nd;
    const RgLightBufDev *lb = nullptr;  // light-buffer descriptors (LDS copy, hot tables)
    const RgLightDev *lt = nullptr;     // lights (LDS copy)
    __device__ __forceinline__ RgBvhNode getn_uniform(int i) const { return nd[i]; }
    __device__ __forceinline__ RgBvhNode getn(int i) const { return nd[i]; }
    __device__ __forceinline__ RgSph getv(int i) const { return s[i]; }
    __device__ __forceinline__ RgPln getp(int i) const { return pl[i]; }
    __device__ __forceinline__ RgDsk getd(int i) const { return dk[i]; }
    __device__ __forceinline__ RgBox getb(int i) const { return bx[i]; }
    __device__ __forceinline__ RgSph get(int i) const { return s[i]; }
    __device__ __forceinline__ double getcc(int i) const { return cc[i]; }
    __device__ __forceinline__ RgSphF getf(int i) const { return f[i]; }
    __device__ __forceinline__ RgSphF2 getf2(int i) const { return f2[i]; }
};

// ---------------------------------------------------------------- f32 pre-filter
// Heavy scenes first test every sphere in f32 (FMA allowed, 2 cycles per wave
// instruction vs 4 for f64) against an INFLATED threshold, and run the exact
// reference test (f64, unfused, bodies.rs:92-119) only for candidates, so the
// accepted set and every distance are bit-identical to the reference.
//
// Bound (u = 2^-24, P_k = |c_k| + |o_k|, S_pp = sum P_k^2, S_p = sum P_k |d_k|):
// with c, o, d rounded to f32, h = c - o, adj = h.d and hh = h.h as FMA chains
// and opp = fma(-adj, adj, hh):
//   |opp32 - OPP| <= u (8.002 S_pp + 13.004 S_p^2)   (f32 path, vs exact reals)
//   |opp64 - OPP| <= 2^-53 (6.02 S_pp + 10.04 S_p^2) (the reference's f64 path)
// and S_pp <= 2(|c|^2 + |o|^2), S_p^2 <= S_pp |d|^2, hence
//   |opp32 - opp64| <= Kd (|c|^2 + |o|^2),  Kd = u (16.2 + 26.2 |d|^2) (rounded up, +1%).
// "miss" is declared only if opp32 > r2hi + Kd(|c|^2 + |o|^2) with r2hi >= r2
// (rounded up on the host with 4u slack, which also covers the two f32
// roundings of the threshold), so opp64 > r2 there: the exact test would
// reject too.  NaN/inf anywhere makes the comparison false -> candidate.
struct RayF {
    float ox, oy, oz, dx, dy, dz;
    float kd;    // Kd for this ray
    float kdo2;  // Kd * |o|^2 (rounded up)
};
__device__ __forceinline__ RayF make_rayf(V3 o, V3 d) {
    RayF r;
    r.ox = (float)o.x; r.oy = (float)o.y; r.oz = (float)o.z;
    r.dx = (float)d.x; r.dy = (float)d.y; r.dz = (float)d.z;
    const float d2 = (float)dot(d, d) * 1.000001f;   // >= |d|^2
    const float o2 = (float)dot(o, o) * 1.000001f;   // >= |o|^2
    r.kd = 5.9604645e-08f * (16.2f + 26.2f * d2) * 1.01f;
    r.kdo2 = r.kd * o2 * 1.000001f;
    return r;
}
// true: the exact test may accept this sphere (run it); false: certain miss
__device__ __forceinline__ bool filter_general(const RgSphF &f, const RgSphF2 &f2, const RayF &r) {
    const float hx = f.cx - r.ox, hy = f.cy - r.oy, hz = f.cz - r.oz;
    const float adj = __builtin_fmaf(hz, r.dz, __builtin_fmaf(hy, r.dy, hx * r.dx));
    const float hh = __builtin_fmaf(hz, hz, __builtin_fmaf(hy, hy, hx * hx));
    const float opp = __builtin_fmaf(-adj, adj, hh);
    const float thr = __builtin_fmaf(r.kd, f2.cchi, f.r2hi + r.kdo2);
    return !(opp > thr);
}
// primary rays: o = 0 and |d|^2 <= 1.00001, so the threshold is a per-sphere
// constant (thrp, host-precomputed) and h.h = fl32(c.c) (cc32)
__device__ __forceinline__ bool filter_primary(const RgSphF &f, const RgSphF2 &f2, float dx, float dy, float dz) {
    const float adj = __builtin_fmaf(f.cz, dz, __builtin_fmaf(f.cy, dy, f.cx * dx));
    const float opp = __builtin_fmaf(-adj, adj, f2.cc32);
    return !(opp > f2.thrp);
}

#ifndef RG_SPH_GROUP
#define RG_SPH_GROUP 2     // spheres per exact miss-test group (one divergent branch per group)
#endif
#define RG_FILTER_GROUP 4  // spheres per f32-filter group (2 and 8 measured slower)

// Primary rays start at the origin (ray.rs:53): h = c - 0 = c exactly, so
// h.h = c.c is a per-sphere constant (bit-identical): 8 FP64 ops per sphere.
template <int G, class Src>
__device__ __forceinline__ void sph_primary_group(const RgKernelArgs &a, const Src &src, int i, V3 d, Closest &c) {
    RgSph s[G];
    double cc[G], adj[G], opp[G];
    bool cand[G];
    bool any = false;
    RG_REGION(RGR_PRIM_GROUP);
#pragma unroll
    for (int k = 0; k < G; ++k) { s[k] = src.get(i + k); cc[k] = src.getcc(i + k); }
#pragma unroll
    for (int k = 0; k < G; ++k) {
        adj[k] = (s[k].cx * d.x + s[k].cy * d.y) + s[k].cz * d.z;
        opp[k] = cc[k] - adj[k] * adj[k];
        cand[k] = !(opp[k] > s[k].r2);   // bodies.rs:99
        any |= cand[k];
    }
    if (any) {
        RG_REGION(RGR_PRIM_SPH_TAIL);
#pragma unroll
        for (int k = 0; k < G; ++k) {
            double t;
#ifdef RG_REGION_STATS
            if (cand[k]) RG_REGION(RGR_PRIM_PAIR);
#endif
            if (cand[k] && sphere_tail(s[k].r2, opp[k], adj[k], t)) closest_add(c, t, rg_cptr(a.sph_id)[i + k]);
        }
    }
}

// f32-filtered primary group: exact f64 work only for candidate spheres
template <int G, class Src>
__device__ __forceinline__ void sph_primary_group_f(const RgKernelArgs &a, const Src &src, int i, V3 d, float dx,
                                                    float dy, float dz, Closest &c) {
    // the group's filter results are OR-ed into one lane predicate (lane masks
    // stay in SGPRs); the rare candidate branch re-evaluates the filter per
    // sphere instead of keeping G per-lane flags alive
    bool any = false;
#pragma unroll
    for (int k = 0; k < G; ++k) any |= filter_primary(src.getf(i + k), src.getf2(i + k), dx, dy, dz);
    if (any) {
#pragma unroll
        for (int k = 0; k < G; ++k) {
            if (filter_primary(src.getf(i + k), src.getf2(i + k), dx, dy, dz)) {
                const RgSph s = src.get(i + k);
                const double cc = src.getcc(i + k);
                const double adj = (s.cx * d.x + s.cy * d.y) + s.cz * d.z;
                const double opp = cc - adj * adj;
                double t;
                if (!(opp > s.r2) && sphere_tail(s.r2, opp, adj, t)) closest_add(c, t, rg_cptr(a.sph_id)[i + k]);
            }
        }
    }
}

template <bool F32F, class Src>
__device__ __forceinline__ void sph_primary(const RgKernelArgs &a, const Src &src, V3 d, Closest &c) {
    if constexpr (F32F) {
        constexpr int G = RG_FILTER_GROUP;
        const float dx = (float)d.x, dy = (float)d.y, dz = (float)d.z;
        const int n = a.n_sph, nfull = n - n % G;
        int i = 0;
        for (; i < nfull; i += G) sph_primary_group_f<G>(a, src, i, d, dx, dy, dz, c);
        for (; i < n; ++i) sph_primary_group_f<1>(a, src, i, d, dx, dy, dz, c);
        return;
    }
    constexpr int G = RG_SPH_GROUP;
    const int n = a.n_sph, nfull = n - n % G;
    int i = 0;
    for (; i < nfull; i += G) sph_primary_group<G>(a, src, i, d, c);
    for (; i < n; ++i) sph_primary_group<1>(a, src, i, d, c);
}

// General rays: closest-hit (secondary) or any-hit (shadow; see trace_query).
template <int G, class Src>
__device__ __forceinline__ void sph_query_group(const RgKernelArgs &a, const Src &src, int i, V3 o, V3 d,
                                                bool shadow, double ld, Closest &c, bool &occl, bool &need) {
    RgSph s[G];
    double adj[G], opp[G];
    bool cand[G];
    bool any = false;
    RG_REGION(RGR_QC_GROUP);
#pragma unroll
    for (int k = 0; k < G; ++k) s[k] = src.get(i + k);
#pragma unroll
    for (int k = 0; k < G; ++k) {
        double hx = s[k].cx - o.x, hy = s[k].cy - o.y, hz = s[k].cz - o.z;     // bodies.rs:92
        adj[k] = (hx * d.x + hy * d.y) + hz * d.z;                              // :93
        opp[k] = ((hx * hx + hy * hy) + hz * hz) - adj[k] * adj[k];             // :95
        cand[k] = !(opp[k] > s[k].r2);                                          // :97-101
        any |= cand[k];
    }
    if (any && need) {
        RG_REGION(RGR_QC_TAIL);
#pragma unroll
        for (int k = 0; k < G; ++k) {
            double t;
#ifdef RG_REGION_STATS
            if (cand[k]) RG_REGION(RGR_QC_PAIR);
#endif
            if (cand[k] && sphere_tail(s[k].r2, opp[k], adj[k], t)) {
                if (shadow) {
                    if (!(t > ld)) { occl = true; need = false; }
                } else {
                    closest_add(c, t, rg_cptr(a.sph_id)[i + k]);
                }
            }
        }
    }
}

template <int G, class Src>
__device__ __forceinline__ void sph_query_group_f(const RgKernelArgs &a, const Src &src, int i, V3 o, V3 d,
                                                  const RayF &rf, bool shadow, double ld, Closest &c, bool &occl,
                                                  bool &need) {
    bool any = false;
#pragma unroll
    for (int k = 0; k < G; ++k) any |= filter_general(src.getf(i + k), src.getf2(i + k), rf);
    if (any && need) {
#pragma unroll
        for (int k = 0; k < G; ++k) {
            if (need && filter_general(src.getf(i + k), src.getf2(i + k), rf)) {
                const RgSph s = src.get(i + k);
                const double hx = s.cx - o.x, hy = s.cy - o.y, hz = s.cz - o.z;
                const double adj = (hx * d.x + hy * d.y) + hz * d.z;
                const double opp = ((hx * hx + hy * hy) + hz * hz) - adj * adj;
                double t;
                if (!(opp > s.r2) && sphere_tail(s.r2, opp, adj, t)) {
                    if (shadow) {
                        if (!(t > ld)) { occl = true; need = false; }
                    } else {
                        closest_add(c, t, rg_cptr(a.sph_id)[i + k]);
                    }
                }
            }
        }
    }
}

template <bool F32F, class Src>
__device__ __forceinline__ bool sph_query(const RgKernelArgs &a, const Src &src, V3 o, V3 d, bool shadow, double ld,
                                          Closest &c, bool &occl, bool &need) {
    if constexpr (F32F) {
        constexpr int G = RG_FILTER_GROUP;
        const RayF rf = make_rayf(o, d);
        const int n = a.n_sph, nfull = n - n % G;
        int i = 0;
        for (; i < nfull; i += G) {
            sph_query_group_f<G>(a, src, i, o, d, rf, shadow, ld, c, occl, need);
            if (((i / G) & 3) == 3 && !__any(need)) return false;
        }
        for (; i < n; ++i) sph_query_group_f<1>(a, src, i, o, d, rf, shadow, ld, c, occl, need);
        return __any(need);
    }
    constexpr int G = RG_SPH_GROUP;
    const int n = a.n_sph, nfull = n - n % G;
    int i = 0;
    for (; i < nfull; i += G) {
        sph_query_group<G>(a, src, i, o, d, shadow, ld, c, occl, need);
        if (((i / G) & 1) && !__any(need)) return false;
    }
    for (; i < n; ++i) sph_query_group<1>(a, src, i, o, d, shadow, ld, c, occl, need);
    return __any(need);
}

}  // namespace rgk
