// rg_shadow_vol.cpp — the shadow mask volume of the PLAIN light kernels (rg_shadow_vol.h).
//
// A light-path hit traces its lights' shadow rays as one batch against every sphere and plane of
// the scene (rg_k_trace.h trace_shadow).  The volume tells a wave which of them can matter: a
// uniform g^3 grid over [-O, O]^3, one u32 per cell, bit i = sphere i, bit 16 + j = plane j.  The
// kernel looks up the cell of each shadow origin, ORs the words over the wave and walks the set
// bits.  It depends on the scene alone and is built once, in rg_scene_create.
//
// CONTRACT.  A bit may be clear in a cell only if the exact test (bodies.rs:92-119 spheres,
// :136-148 planes, with the shadow acceptance !(t > light distance), rendering.rs:152-155) cannot
// accept that body for any shadow ray that starts in the cell and goes towards any light.
//
// SETTING.  S = largest |coordinate| of any sphere bound, O = 4 S + 1 (as rg_bvh.cpp), cell edge
// e = 2 O / g, cell centre b, half-diagonal rho = e sqrt(3) / 2, margin m = 2^-16 (S + O) >= 2^-16.
// Every scene parameter is finite and at most 2^20 in magnitude (rg_shadow_vol_admits), so
// S + O < 2^24.  A shadow ray starts at o = h + n 1e-13 (h the hit, n its unit normal) with the
// direction d and the light distance ld of light_dir_dist(h): d = dn, ld = inf (directional) or
// d = fl((L - h) / |L - h|), ld = fl(|L - h|) (spherical), |d - u| <= 2^-50 for the true unit vector u.
// Only origins with a cell are concerned (the others take the all-ones word), so |o_k| <= O (1 + 2^-22).
//
//  (a) Cell.  rg_shvol_cell displaces o by at most 2^-22 O (rg_shadow_vol_cell.h), and |o - h| =
//      1e-13: the ray's cell contains a point within delta = 2^-22 O + 1e-13 of h and of o, so
//      |o - b| <= rho + delta, |h - b| <= rho + delta.
//  (b) Cell ball.  For o in ball(b, R) the point of the segment [o, L] at parameter s lies within
//      (1 - s) R of the point of [b, L] at s; for a direction dn the point o + t dn lies within R
//      of b + t dn.  So the ray's points are within R of the segment [b, L], or of the half-line
//      {b + t dn, t >= 0}.
//  (c) Spheres.  An accepted hit has a computed t in [0, ld] (bodies.rs:105-118 returns no negative
//      distance) and opp <= r^2.  With th^2 = r^2 - opp, the point p = o + t d has |p - c|^2 = r^2 +
//      (the rounding of opp and th), which is at most 2^-47 (S + O)^2: |p - c| <= r + 2^-23.5 (S + O)
//      (rg_bvh.cpp's bound).  For a spherical light o + ld d = L + (o - h) up to rounding, so p is within
//      2^-30 of [o, L].  Hence dist(c, [b, L]) <= r + rho + delta + 2^-23.5 (S + O) + 2^-30
//      < r + rho + m; for a directional light the same with the half-line.  The builder sets the
//      bit where its own f64 evaluation of that distance (error below 2^-28) is <= r + rho + 2 m.
//      A light inside or near a sphere needs no case of its own: [b, L] then passes within r of c.
//  (d) Planes, any light.  The test accepts only if den = fl(n . d) > 1e-6 and dist = fl(num / den)
//      satisfies dist >= 0 and !(dist > ld), num = fl((p_o - o) . n).  Write N = |n|, a = n . u / N,
//      q = n . (p_o - o) / N.  Dot-product rounding: den = N (a +- 2^-49), num = N (q +- e1),
//      e1 = 2^-51 (2^21 + O) < 2^-27.
//  (d1) Directional light: den is one number per (plane, light), evaluated here exactly as the
//      kernel does (unfused, same order, d = RgLightDev::dn).  Where it is not > 1e-6 the pair is
//      out for every cell.
//  (d2) Spherical light strictly on the -n side of the plane, n . (p_o - L) / N >= m: out for every
//      cell.  If q - e1 < 0 then num < 0 and dist < 0.  Otherwise ld a N = n . (L - h) gives
//      q = ld a + n . (p_o - L) / N + n . (h - o) / N >= ld a + m - 1e-13, and
//      dist >= (q - e1) / (a + 2^-49) (1 - 2^-53) > ld (1 + 2^-52) >= fl(ld), because
//      m - 1e-13 - e1 > ld 2^-48 (ld < 2^22): the crossing lies behind the light.
//  (d3) Spherical light, per cell: out where n . (L - b) / N <= -(rho + m).  Then n . (L - h) / N
//      <= -(m - delta) < -2^-17, a <= -2^-17 / 2^22 = -2^-39, and den = N (a +- 2^-49) < 0.
//  Anything else keeps the bit.  The builder's own f64 rounding (below 2^-28 in these distances) is
//  inside the slack between m and what (a) .. (d) need.
//
// Built in two levels: a block of 8^3 cells is tested first with its own half-diagonal (a cell
// centre is within rho_block - rho of the block's, so by (b) a pair that fails r + rho_block + 2 m
// at the block centre fails at every cell of it); only the pairs that pass are tested per cell.
#if defined(__HIP__)
#include <hip/hip_runtime.h>  // hipcc builds this file as HIP (host code only)
#endif
#include "rg_shadow_vol.h"

#include <algorithm>
#include <chrono>
#include <cmath>

#include "../../include/raingun.h"
#include "rg_device.h"

namespace {

double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// squared distance of c from the segment [b, L]
double seg_dist2(const double *c, const double *b, const double *L) {
    const double p[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]};
    const double e[3] = {L[0] - b[0], L[1] - b[1], L[2] - b[2]};
    const double ee = dot3(e, e);
    double t = ee > 0.0 ? dot3(p, e) / ee : 0.0;
    t = std::min(std::max(t, 0.0), 1.0);
    const double w[3] = {p[0] - t * e[0], p[1] - t * e[1], p[2] - t * e[2]};
    return dot3(w, w);
}

// squared distance of c from the half-line {b + t d, t >= 0}, |d| = 1 up to rounding
double ray_dist2(const double *c, const double *b, const double *d) {
    const double p[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]};
    const double t = std::max(dot3(p, d) / dot3(d, d), 0.0);
    const double w[3] = {p[0] - t * d[0], p[1] - t * d[1], p[2] - t * d[2]};
    return dot3(w, w);
}

bool small_finite(double v) { return std::isfinite(v) && std::fabs(v) <= RG_SHVOL_MAX_MAG; }

#ifdef RG_SHVOL_TEST_NO_MARGIN  // negative control of tests/test_shadow_vol_cpu.py: must be caught
constexpr double kShrink = 0.99, kMargin = 0.0;
#else
constexpr double kShrink = 1.0, kMargin = 1.0;
#endif

}  // namespace

bool rg_shadow_vol_admits(const double *spheres, int n_sph, const double *planes, int n_pln,
                          const RgShadowVolLight *lights, int n_lights) {
    if (n_sph < 0 || n_pln < 0 || n_sph + n_pln < 1 || n_sph > RG_SHVOL_MAX_BODIES || n_pln > RG_SHVOL_MAX_BODIES)
        return false;
    if (n_lights < 1 || n_lights > RG_LB) return false;
    for (int i = 0; i < 4 * n_sph; ++i)
        if (!small_finite(spheres[i])) return false;
    for (int i = 0; i < 6 * n_pln; ++i)
        if (!small_finite(planes[i])) return false;
    for (int l = 0; l < n_lights; ++l)
        for (int k = 0; k < 3; ++k) {
            if (!small_finite(lights[l].v[k])) return false;
            if (lights[l].kind == RG_LIGHT_DIRECTIONAL && !small_finite(lights[l].dn[k])) return false;
        }
    return true;
}

bool rg_build_shadow_vol(const double *spheres, int n_sph, const double *planes, int n_pln,
                         const RgShadowVolLight *lights, int n_lights, int g, RgShadowVolBuild &out) {
    out = RgShadowVolBuild();
    if (g < 1 || g > RG_SHVOL_MAX_G || !rg_shadow_vol_admits(spheres, n_sph, planes, n_pln, lights, n_lights))
        return false;
    const auto t0 = std::chrono::steady_clock::now();
    double S = 0.0;
    for (int i = 0; i < n_sph; ++i) {
        const double *p = spheres + 4 * i, r = std::fabs(p[3]);
        for (int k = 0; k < 3; ++k) S = std::max(S, std::max(std::fabs(p[k] - r), std::fabs(p[k] + r)));
    }
    const double O = 4.0 * S + 1.0;
    const double m = kMargin * 1.52587890625e-05 * (S + O);  // 2^-16 (S + O)
    const double e = 2.0 * O / (double)g;
    const double rho = kShrink * e * 0.8660254037844387;  // sqrt(3) / 2, rounded up
    constexpr int B = 8;
    const double rho_block = rho + (double)(B - 1) * e * 0.8660254037844387;  // block centre to a cell centre + rho

    // planes: the pairs that are out everywhere (d1, d2); `cellwise` lists the spherical pairs left (d3)
    uint32_t plane_all = 0u;  // planes some directional light keeps: set in every cell
    struct PlanePair { int j; double nl[3], thr; };
    std::vector<PlanePair> cellwise;
    for (int j = 0; j < n_pln; ++j) {
        const double *po = planes + 6 * j, *n = po + 3;
        const double N = std::sqrt(dot3(n, n));
        for (int l = 0; l < n_lights; ++l) {
            const RgShadowVolLight &L = lights[l];
            if (L.kind == RG_LIGHT_DIRECTIONAL) {
                const double den = (n[0] * L.dn[0] + n[1] * L.dn[1]) + n[2] * L.dn[2];  // the kernel's expression
                if (den > 1e-6) plane_all |= 1u << (16 + j);
                continue;
            }
            if (!(N > 0.0)) continue;  // den = 0 for every ray
            const double v[3] = {po[0] - L.v[0], po[1] - L.v[1], po[2] - L.v[2]};
            if (dot3(n, v) / N >= m) continue;  // (d2)
            // (d3) out where n . (L - b) / N <= -(rho + m)  <=>  n . b / N >= n . L / N + rho + m
            cellwise.push_back(PlanePair{j, {n[0] / N, n[1] / N, n[2] / N}, dot3(n, L.v) / N + rho + m});
        }
    }

    out.words.assign((size_t)g * g * g, plane_all);
    struct Pair { int i, l; };
    std::vector<Pair> live;
    live.reserve((size_t)n_sph * n_lights);
    auto centre = [&](int k) { return -O + ((double)k + 0.5) * e; };
    auto sphere_near = [&](int i, int l, const double *b, double reach) {
        const double *c = spheres + 4 * i;
        const RgShadowVolLight &L = lights[l];
        const double thr = kShrink * std::fabs(c[3]) + reach + 2.0 * m;
        const double d2 = L.kind == RG_LIGHT_DIRECTIONAL ? ray_dist2(c, b, L.dn) : seg_dist2(c, b, L.v);
        return d2 <= thr * thr;
    };
    for (int bz = 0; bz < g; bz += B)
        for (int by = 0; by < g; by += B)
            for (int bx = 0; bx < g; bx += B) {
                // the block of B^3 cell slots at (bx, by, bz) (cells past g are not visited: the
                // centre and half-diagonal of the whole block still bound the ones that are)
                const double bb[3] = {-O + ((double)bx + 0.5 * B) * e, -O + ((double)by + 0.5 * B) * e,
                                      -O + ((double)bz + 0.5 * B) * e};
                live.clear();
                for (int i = 0; i < n_sph; ++i)
                    for (int l = 0; l < n_lights; ++l)
                        if (sphere_near(i, l, bb, rho_block)) live.push_back(Pair{i, l});
                if (live.empty() && cellwise.empty()) continue;
                for (int z = bz; z < std::min(bz + B, g); ++z)
                    for (int y = by; y < std::min(by + B, g); ++y)
                        for (int x = bx; x < std::min(bx + B, g); ++x) {
                            const double b[3] = {centre(x), centre(y), centre(z)};
                            uint32_t w = 0u;
                            for (const Pair &p : live)
                                if (!((w >> p.i) & 1u) && sphere_near(p.i, p.l, b, rho)) w |= 1u << p.i;
                            for (const PlanePair &p : cellwise)
                                if (!(dot3(p.nl, b) >= p.thr)) w |= 1u << (16 + p.j);
                            out.words[((size_t)z * g + y) * g + x] |= w;
                        }
            }
    unsigned long long set = 0;
    for (uint32_t w : out.words) set += (unsigned long long)__builtin_popcount(w);
    out.g = g;
    out.inv = (float)((double)g / (2.0 * O));
    out.off = 0.5f * (float)g;
    out.extent = S;
    out.obound = O;
    out.margin = m;
    out.set_share = (double)set / ((double)out.words.size() * (double)(n_sph + n_pln));
    out.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return true;
}
