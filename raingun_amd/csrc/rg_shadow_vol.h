// rg_shadow_vol.h — host-side builder of the shadow mask volume of the PLAIN light kernels
// (rg_shadow_vol.cpp; cell lookup: rg_shadow_vol_cell.h).
//
// Like the light buffers (rg_lightbuf.h) it only decides which bodies a shadow ray tests with the
// exact reference test: a body's bit is clear in a cell only if that test cannot accept the body for
// any shadow ray that starts in the cell, so every shadow answer is the full scan's.
#pragma once
#include <cstdint>
#include <vector>

#include "rg_shadow_vol_cell.h"

#ifndef RG_SHVOL_G
#define RG_SHVOL_G 64  // cells per axis: 1 MiB of u32 words
#endif
#define RG_SHVOL_MAX_G 256
// every sphere, plane and light parameter of an admitted scene is at most this in magnitude
// (the rounding bounds of the proof in rg_shadow_vol.cpp are stated for it)
#define RG_SHVOL_MAX_MAG 1048576.0  // 2^20

struct RgShadowVolLight {
    int kind;      // RG_LIGHT_DIRECTIONAL / RG_LIGHT_SPHERICAL
    double v[3];   // direction / position
    double dn[3];  // directional: normalize(-direction) as RgLightDev::dn holds it
};

struct RgShadowVolBuild {
    std::vector<uint32_t> words;  // g^3 cells, x fastest
    int g = 0;
    float inv = 0.0f, off = 0.0f;  // rg_shvol_cell's constants
    double extent = 0.0, obound = 0.0, margin = 0.0;  // S, O = 4 S + 1, m = 2^-16 (S + O)
    double build_ms = 0.0;
    double set_share = 0.0;  // set bits / (cells x bodies)
};

// May the scene have a volume?  At least one sphere or plane, at most RG_SHVOL_MAX_BODIES of each,
// 1 .. RG_LB lights, every parameter finite and at most RG_SHVOL_MAX_MAG in magnitude.
// spheres: n_sph x (centre xyz, radius); planes: n_pln x (origin xyz, normal xyz), both in the
// kernel's table order.
bool rg_shadow_vol_admits(const double *spheres, int n_sph, const double *planes, int n_pln,
                          const RgShadowVolLight *lights, int n_lights);

// The volume of an admitted scene with g cells per axis (false: not admitted, or g out of range).
bool rg_build_shadow_vol(const double *spheres, int n_sph, const double *planes, int n_pln,
                         const RgShadowVolLight *lights, int n_lights, int g, RgShadowVolBuild &out);
