// shadow_vol_sim.cpp — CPU check that the shadow mask volume (raingun_amd/csrc/rg_shadow_vol.cpp)
// never clears the bit of a body the exact reference test would accept: for every shadow ray and
// every body, if the exact test accepts the body (hit, and !(t > light distance)), the body's bit is
// set in the word of the ray's cell (cell lookup: the kernel's own rg_shadow_vol_cell.h).  Built and
// run by tests/test_shadow_vol_cpu.py.
//
// usage: shadow_vol_sim rays g [fov] < scene.txt
//   scene.txt: n, n lines "cx cy cz r"; p, p lines "ox oy oz nx ny nz"; m, m lines "kind x y z"
//   (kind 0 = directional with direction xyz, 1 = spherical at position xyz)
//   fov (degrees) given: also the kept fractions per 8x8 tile of the primary hits at 960x536
// Prints one JSON line; exit 1 on any violation, 3 if the scene is not admitted.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/raingun.h"
#include "../../raingun_amd/csrc/rg_shadow_vol.h"

static std::vector<double> sp, pl;  // 4 per sphere, 6 per plane
static std::vector<RgShadowVolLight> lights;
static int n_sph = 0, n_pln = 0;
static RgShadowVolBuild vol;
static long g_rays = 0, g_accept = 0, g_viol = 0, g_nocell = 0, g_grazing = 0, g_lattice = 0;

// bodies.rs:92-119 (f64, unfused; compiled with -ffp-contract=off)
static bool sphere_exact(const double *s, const double o[3], const double d[3], double &t) {
    const double hx = s[0] - o[0], hy = s[1] - o[1], hz = s[2] - o[2];
    const double adj = (hx * d[0] + hy * d[1]) + hz * d[2];
    const double opp = ((hx * hx + hy * hy) + hz * hz) - adj * adj;
    const double r2 = s[3] * s[3];
    if (opp > r2) return false;
    const double th = std::sqrt(r2 - opp);
    const double d0 = adj - th, d1 = adj + th;
    if (d0 < 0.0 && d1 < 0.0) return false;
    t = d0 < 0.0 ? d1 : (d1 < 0.0 ? d0 : std::fmin(d0, d1));
    return true;
}
// bodies.rs:136-148
static bool plane_exact(const double *p, const double o[3], const double d[3], double &t) {
    const double den = (p[3] * d[0] + p[4] * d[1]) + p[5] * d[2];
    if (!(den > 1e-6)) return false;
    const double vx = p[0] - o[0], vy = p[1] - o[1], vz = p[2] - o[2];
    t = ((vx * p[3] + vy * p[4]) + vz * p[5]) / den;
    return t >= 0.0;
}

static uint64_t rng_state = 0x5EEDULL;
static double urand() {  // SplitMix64 -> [0, 1)
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
static void unit(double v[3]) {
    const double inv = 1.0 / std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    v[0] *= inv; v[1] *= inv; v[2] *= inv;
}
static void rand_dir(double v[3]) {
    do { for (int k = 0; k < 3; ++k) v[k] = 2.0 * urand() - 1.0; } while ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2] < 1e-6);
    unit(v);
}
static void cross(const double a[3], const double b[3], double c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// direction and distance towards light l from the hit h, as the kernel's light_dir_dist
static void shadow_ray(const RgShadowVolLight &l, const double h[3], double d[3], double &ld) {
    if (l.kind == RG_LIGHT_DIRECTIONAL) {
        d[0] = l.dn[0]; d[1] = l.dn[1]; d[2] = l.dn[2];
        ld = HUGE_VAL;
        return;
    }
    const double v[3] = {l.v[0] - h[0], l.v[1] - h[1], l.v[2] - h[2]};
    const double m = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const double inv = 1.0 / m;
    d[0] = v[0] * inv; d[1] = v[1] * inv; d[2] = v[2] * inv;
    ld = m;
}

static uint32_t word_of(const double o[3]) {
    const int cell = rg_shvol_cell((float)o[0], (float)o[1], (float)o[2], vol.inv, vol.off, vol.g);
    if (cell == RG_SHVOL_NO_CELL) { ++g_nocell; return RG_SHVOL_ALL; }
    return vol.words[(size_t)cell];
}

// a hit at h with unit normal n: the batch's rays start at o = h + n * 1e-13 (rendering.rs:148)
static void check(const double h[3], const double n[3]) {
    const double o[3] = {h[0] + n[0] * 1e-13, h[1] + n[1] * 1e-13, h[2] + n[2] * 1e-13};
    const uint32_t w = word_of(o);
    for (const RgShadowVolLight &l : lights) {
        double d[3], ld, t;
        shadow_ray(l, h, d, ld);
        ++g_rays;
        for (int i = 0; i < n_sph; ++i)
            if (sphere_exact(&sp[4 * i], o, d, t) && !(t > ld)) {
                ++g_accept;
                if (!((w >> i) & 1u)) {
                    if (g_viol++ < 5)
                        std::fprintf(stderr, "violation: sphere %d light kind %d o=(%.17g %.17g %.17g)\n", i, l.kind, o[0], o[1], o[2]);
                }
            }
        for (int j = 0; j < n_pln; ++j)
            if (plane_exact(&pl[6 * j], o, d, t) && !(t > ld)) {
                ++g_accept;
                if (!((w >> (16 + j)) & 1u)) {
                    if (g_viol++ < 5)
                        std::fprintf(stderr, "violation: plane %d light kind %d o=(%.17g %.17g %.17g)\n", j, l.kind, o[0], o[1], o[2]);
                }
            }
    }
}
static void check(const double h[3]) {
    double n[3];
    rand_dir(n);
    check(h, n);
}

int main(int argc, char **argv) {
    const int R = argc > 1 ? std::atoi(argv[1]) : 3000;
    const int G = argc > 2 ? std::atoi(argv[2]) : RG_SHVOL_G;
    const double fov = argc > 3 ? std::atof(argv[3]) : 0.0;
    if (std::scanf("%d", &n_sph) != 1 || n_sph < 0) return 2;
    sp.resize(4 * (size_t)n_sph);
    for (double &v : sp)
        if (std::scanf("%lf", &v) != 1) return 2;
    if (std::scanf("%d", &n_pln) != 1 || n_pln < 0) return 2;
    pl.resize(6 * (size_t)n_pln);
    for (double &v : pl)
        if (std::scanf("%lf", &v) != 1) return 2;
    int m;
    if (std::scanf("%d", &m) != 1 || m < 0) return 2;
    lights.resize(m);
    for (auto &l : lights) {
        int k;
        if (std::scanf("%d %lf %lf %lf", &k, &l.v[0], &l.v[1], &l.v[2]) != 4) return 2;
        l.kind = k == 0 ? RG_LIGHT_DIRECTIONAL : RG_LIGHT_SPHERICAL;
        const double nx = -l.v[0], ny = -l.v[1], nz = -l.v[2];  // as rg_scene.hip computes RgLightDev::dn
        const double inv = 1.0 / std::sqrt((nx * nx + ny * ny) + nz * nz);
        l.dn[0] = nx * inv; l.dn[1] = ny * inv; l.dn[2] = nz * inv;
    }
    if (!rg_build_shadow_vol(sp.data(), n_sph, pl.data(), n_pln, lights.data(), m, G, vol)) {
        std::printf("{\"admitted\": 0}\n");
        return 3;
    }
    const double O = vol.obound, e = 2.0 * O / G;
    // (plane, directional light) pairs whose den lies within a few ulps of the test's 1e-6
    int den_near = 0;
    for (int j = 0; j < n_pln; ++j)
        for (const auto &l : lights) {
            const double den = (pl[6 * j + 3] * l.dn[0] + pl[6 * j + 4] * l.dn[1]) + pl[6 * j + 5] * l.dn[2];
            den_near += l.kind == RG_LIGHT_DIRECTIONAL && std::fabs(den - 1e-6) < 1e-6 * 3.6e-15;
        }
    for (int r = 0; r < R; ++r) {
        double h[3], n[3];
        // 1. hits on sphere surfaces, the origin pushed out along the normal by the shadow bias
        if (n_sph > 0) {
            const double *s = &sp[4 * (int)(urand() * n_sph)];
            rand_dir(n);
            for (int k = 0; k < 3; ++k) h[k] = s[k] + n[k] * std::fabs(s[3]);
            check(h, n);
        }
        // 2. hits on the planes, shaded from either side
        if (n_pln > 0) {
            const double *p = &pl[6 * (int)(urand() * n_pln)];
            double nn[3] = {p[3], p[4], p[5]}, w[3], u[3], v[3];
            if ((nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2] > 0.0) {
                unit(nn);
                do { rand_dir(w); cross(nn, w, u); } while ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2] < 1e-3);
                unit(u);
                cross(nn, u, v);
                const double a = (2.0 * urand() - 1.0) * 1.2 * O, b = (2.0 * urand() - 1.0) * 1.2 * O;
                for (int k = 0; k < 3; ++k) h[k] = p[k] + a * u[k] + b * v[k];
                const double sgn = urand() < 0.5 ? -1.0 : 1.0;
                for (int k = 0; k < 3; ++k) n[k] = sgn * nn[k];
                check(h, n);
            }
        }
        // 3. random points in the domain, and in a cube 3x its size (outside: the all-ones word)
        for (int k = 0; k < 3; ++k) h[k] = (2.0 * urand() - 1.0) * O;
        check(h);
        for (int k = 0; k < 3; ++k) h[k] = (2.0 * urand() - 1.0) * 3.0 * O;
        check(h);
        if (n_sph > 0) {  // ... and near the spheres
            const double *s = &sp[4 * (int)(urand() * n_sph)];
            for (int k = 0; k < 3; ++k) h[k] = s[k] + (2.0 * urand() - 1.0) * (3.0 * std::fabs(s[3]) + 2.0 * e);
            check(h);
        }
        // 4. grazing: the shadow ray passes at r (1 +- eps) from a sphere's centre
        for (const auto &l : lights) {
            if (n_sph == 0) break;
            const double *s = &sp[4 * (int)(urand() * n_sph)];
            const double rr = std::fabs(s[3]) * (1.0 + (urand() < 0.5 ? -1.0 : 1.0) * (urand() < 0.5 ? 1e-9 : 1e-13));
            if (l.kind == RG_LIGHT_DIRECTIONAL) {
                double u[3], w[3];
                do { rand_dir(w); cross(l.dn, w, u); } while ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2] < 1e-3);
                unit(u);
                const double back = std::fabs(s[3]) + 0.5 * O * urand();  // the sphere ahead of o along dn
                for (int k = 0; k < 3; ++k) h[k] = s[k] + rr * u[k] - back * l.dn[k];
            } else {
                double c_l[3] = {s[0] - l.v[0], s[1] - l.v[1], s[2] - l.v[2]};
                const double D = std::sqrt(c_l[0] * c_l[0] + c_l[1] * c_l[1] + c_l[2] * c_l[2]);
                if (!(D > rr * 1.01)) continue;
                unit(c_l);
                double w[3], u[3], dir[3];
                do { rand_dir(w); cross(c_l, w, u); } while ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2] < 1e-3);
                unit(u);
                const double th = std::asin(rr / D);  // a ray from L tangent to the (r (1 +- eps)) sphere
                for (int k = 0; k < 3; ++k) dir[k] = std::cos(th) * c_l[k] + std::sin(th) * u[k];
                const double reach = D * std::cos(th) * (1.0 + 2.0 * urand()) + std::fabs(s[3]);
                for (int k = 0; k < 3; ++k) h[k] = l.v[k] + reach * dir[k];
            }
            ++g_grazing;
            check(h);
        }
    }
    // 5. origins on cell faces and corners: the lattice points of every cell within two cells of a
    // sphere's box (at most 40^3 per sphere) and of random cells -- the point itself, points a hair
    // inside each of the eight cells that meet there, and the face centres next to it
    auto lattice = [&](int ix, int iy, int iz) {
        const double c[3] = {-O + ix * e, -O + iy * e, -O + iz * e};
        check(c);
        for (const double hair : {1e-9, 1e-4})  // below and above what the lookup's f32 resolves
            for (int s = 0; s < 8; ++s) {
                const double h[3] = {c[0] + ((s & 1) ? hair : -hair) * e, c[1] + ((s & 2) ? hair : -hair) * e,
                                     c[2] + ((s & 4) ? hair : -hair) * e};
                check(h);
            }
        for (int k = 0; k < 3; ++k) {
            double h[3] = {c[0] + 0.5 * e, c[1] + 0.5 * e, c[2] + 0.5 * e};
            h[k] = c[k];
            check(h);
        }
        ++g_lattice;
    };
    for (int i = 0; i < n_sph; ++i) {
        int lo[3], hi[3];
        for (int k = 0; k < 3; ++k) {
            lo[k] = std::max(0, (int)std::floor((sp[4 * i + k] - std::fabs(sp[4 * i + 3]) + O) / e) - 2);
            hi[k] = std::min(G, (int)std::floor((sp[4 * i + k] + std::fabs(sp[4 * i + 3]) + O) / e) + 3);
            hi[k] = std::min(hi[k], lo[k] + 40);
        }
        for (int z = lo[2]; z <= hi[2]; ++z)
            for (int y = lo[1]; y <= hi[1]; ++y)
                for (int x = lo[0]; x <= hi[0]; ++x) lattice(x, y, z);
    }
    for (int r = 0; r < R; ++r) lattice((int)(urand() * (G + 1)), (int)(urand() * (G + 1)), (int)(urand() * (G + 1)));

    std::printf("{\"admitted\": 1, \"g\": %d, \"bytes\": %zu, \"build_ms\": %.3f, \"set_share\": %.5f, \"rays\": %ld, "
                "\"accepted\": %ld, \"violations\": %ld, \"no_cell\": %ld, \"grazing\": %ld, \"lattice_points\": %ld, "
                "\"den_near_1e-6\": %d",
                vol.g, vol.words.size() * sizeof(uint32_t), vol.build_ms, vol.set_share, g_rays, g_accept, g_viol, g_nocell,
                g_grazing, g_lattice, den_near);
    if (fov > 0.0) {
        // the primary hits of a 960x536 frame (ray.rs:37-54 from the origin), per 8x8 tile the OR of their cells' words
        const int W = 960, H = 536;
        const double fa = std::tan(fov * (3.14159265358979323846 / 180.0) / 2.0), aspect = (double)W / H;
        long tiles = 0, sph_left = 0, pln_left = 0, hits = 0, hits_on_planes = 0;
        for (int ty = 0; ty < H; ty += 8)
            for (int tx = 0; tx < W; tx += 8) {
                uint32_t mask = 0u;
                bool any = false;
                for (int y = ty; y < std::min(ty + 8, H); ++y)
                    for (int x = tx; x < std::min(tx + 8, W); ++x) {
                        double d[3] = {((((double)x + 0.5) / W) * 2.0 - 1.0) * aspect * fa,
                                       (1.0 - (((double)y + 0.5) / H) * 2.0) * fa, -1.0};
                        unit(d);
                        const double o[3] = {0.0, 0.0, 0.0};
                        double best = HUGE_VAL, t;
                        bool plane = false;
                        for (int i = 0; i < n_sph; ++i)
                            if (sphere_exact(&sp[4 * i], o, d, t) && t < best) { best = t; plane = false; }
                        for (int j = 0; j < n_pln; ++j)
                            if (plane_exact(&pl[6 * j], o, d, t) && t < best) { best = t; plane = true; }
                        if (best == HUGE_VAL) continue;
                        const double h[3] = {d[0] * best, d[1] * best, d[2] * best};
                        const int cell = rg_shvol_cell((float)h[0], (float)h[1], (float)h[2], vol.inv, vol.off, vol.g);
                        mask |= cell == RG_SHVOL_NO_CELL ? RG_SHVOL_ALL : vol.words[(size_t)cell];
                        any = true;
                        ++hits;
                        hits_on_planes += plane;
                    }
                if (!any) continue;
                ++tiles;
                const uint32_t ms = mask & ((1u << n_sph) - 1u), mp = (mask >> 16) & ((1u << n_pln) - 1u);
                sph_left += __builtin_popcount(ms);
                pln_left += __builtin_popcount(mp);
            }
        std::printf(", \"tiles\": %ld, \"sphere_tests_left\": %.4f, \"plane_tests_left\": %.4f, \"hits_on_planes\": %.4f",
                    tiles, n_sph ? (double)sph_left / ((double)tiles * n_sph) : 0.0,
                    n_pln ? (double)pln_left / ((double)tiles * n_pln) : 0.0, hits ? (double)hits_on_planes / hits : 0.0);
    }
    std::printf("}\n");
    return g_viol ? 1 : 0;
}
