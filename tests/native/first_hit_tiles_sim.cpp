// first_hit_tiles_sim.cpp — CPU count of the 8x8 tiles that pass the vote of the PLAIN light kernels'
// first-hit path (raingun_amd/csrc/rg_render_kernel.h): a tile passes if every pixel of
// it inside the frame ends its primary ray at a miss, at a Diffuse body, or at a Reflecting body with
// max_depth <= 1.  The vote depends only on the primary hit's body and max_depth.  Built and run by
// tests/test_first_hit_tiles_cpu.py.
//
// usage: first_hit_tiles_sim width height fov max_depth < scene.txt
//   scene.txt: n, n lines "cx cy cz r surface"; p, p lines "ox oy oz nx ny nz surface"
//   (surface 0 = Diffuse, 1 = Reflecting, 2 = Refractive; a scene of spheres and planes only)
// Prints one JSON line: the frame's tiles, the voting tiles, and the voting tiles per tile row.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

// bodies.rs:92-119 (f64, unfused; compiled with -ffp-contract=off)
static bool sphere_exact(const double *s, const double d[3], double &t) {
    const double hx = s[0], hy = s[1], hz = s[2];  // the ray starts at the origin
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
static bool plane_exact(const double *p, const double d[3], double &t) {
    const double den = (p[3] * d[0] + p[4] * d[1]) + p[5] * d[2];
    if (!(den > 1e-6)) return false;
    t = ((p[0] * p[3] + p[1] * p[4]) + p[2] * p[5]) / den;
    return t >= 0.0;
}

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), max_depth = std::atoi(argv[4]);
    const double fov = std::atof(argv[3]);
    if (W <= 0 || H <= 0 || !(fov > 0.0)) return 2;
    int n_sph = 0, n_pln = 0;
    if (std::scanf("%d", &n_sph) != 1 || n_sph < 0) return 2;
    std::vector<double> sp(5 * (size_t)n_sph);
    for (double &v : sp)
        if (std::scanf("%lf", &v) != 1) return 2;
    if (std::scanf("%d", &n_pln) != 1 || n_pln < 0) return 2;
    std::vector<double> pl(7 * (size_t)n_pln);
    for (double &v : pl)
        if (std::scanf("%lf", &v) != 1) return 2;
    // ray.rs:37-54 from the origin
    const double fa = std::tan(fov * (3.14159265358979323846 / 180.0) / 2.0), aspect = (double)W / H;
    auto simple = [&](int surface) { return surface == 0 || (surface == 1 && 1 >= max_depth); };
    long tiles = 0, voting = 0;
    std::vector<long> rows;
    for (int ty = 0; ty < H; ty += 8) {
        long row = 0;
        for (int tx = 0; tx < W; tx += 8) {
            bool all = true;
            for (int y = ty; y < ty + 8 && y < H; ++y)
                for (int x = tx; x < tx + 8 && x < W; ++x) {
                    double d[3] = {((((double)x + 0.5) / W) * 2.0 - 1.0) * aspect * fa, (1.0 - (((double)y + 0.5) / H) * 2.0) * fa, -1.0};
                    const double inv = 1.0 / std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
                    d[0] *= inv; d[1] *= inv; d[2] *= inv;
                    double best = HUGE_VAL, t;
                    int surface = 0;  // a miss is simple
                    for (int i = 0; i < n_sph; ++i)
                        if (sphere_exact(&sp[5 * i], d, t) && t < best) { best = t; surface = (int)sp[5 * i + 4]; }
                    for (int j = 0; j < n_pln; ++j)
                        if (plane_exact(&pl[7 * j], d, t) && t < best) { best = t; surface = (int)pl[7 * j + 6]; }
                    all = all && simple(surface);
                }
            ++tiles;
            voting += all;
            row += all;
        }
        rows.push_back(row);
    }
    std::printf("{\"tiles\": %ld, \"voting\": %ld, \"rows\": [", tiles, voting);
    for (size_t k = 0; k < rows.size(); ++k) std::printf("%s%ld", k ? ", " : "", rows[k]);
    std::printf("]}\n");
    return 0;
}
