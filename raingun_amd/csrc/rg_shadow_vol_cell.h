// rg_shadow_vol_cell.h — cell lookup of the shadow mask volume (rg_shadow_vol.cpp), shared by the
// PLAIN light kernels (rg_render_kernel.h) and the CPU check (tests/native/shadow_vol_sim.cpp).
// No HIP header: plain C++ on the host, device code where hipcc compiles it.
//
// The volume is a uniform g x g x g grid over [-O, O]^3, one u32 per cell: bit i = sphere position i
// (kernel table order), bit 16 + j = plane j.  A shadow origin o maps to cell
//   (floor(fx), floor(fy), floor(fz)),  f = fma((float)o, inv, off),  inv = fl32(g / 2O),  off = g / 2,
// and to no cell (RG_SHVOL_NO_CELL: the caller takes the all-ones word) when any coordinate is
// non-finite or lands outside [0, g).  Error of the mapping, as a displacement of o: |o| 2^-24 for the
// conversion, |o| 2^-24 for inv's rounding and 2O 2^-24 for the fma's one rounding (f < g), together
// at most 2^-22 O: the builder's margin m = 2^-16 (S + O) covers it (proof: rg_shadow_vol.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define RG_SHVOL_FN __host__ __device__ __forceinline__
#else
#define RG_SHVOL_FN inline
#endif

#define RG_SHVOL_NO_CELL (-1)
#define RG_SHVOL_ALL 0xFFFFFFFFu     // the word of an origin without a cell: every body is tested
#define RG_SHVOL_MAX_BODIES 16       // spheres (bits 0..15) and planes (bits 16..31) a volume can hold

RG_SHVOL_FN int rg_shvol_cell(float ox, float oy, float oz, float inv, float off, int g) {
    const float fx = __builtin_fmaf(ox, inv, off), fy = __builtin_fmaf(oy, inv, off), fz = __builtin_fmaf(oz, inv, off);
    const float fg = (float)g;
    // every comparison is false for a NaN
    const bool in = fx >= 0.0f && fx < fg && fy >= 0.0f && fy < fg && fz >= 0.0f && fz < fg;
    if (!in) return RG_SHVOL_NO_CELL;
    return ((int)fz * g + (int)fy) * g + (int)fx;  // f >= 0: the conversion truncates = floor
}
