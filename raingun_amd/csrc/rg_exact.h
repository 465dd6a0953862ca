// rg_exact.h — exact replacements for divisions whose divisor the host knows before the launch, and
// the host-side checks that admit them.  No HIP include: host code, device code (the PLAIN light
// kernels, rg_render_kernel.h) and the stand-alone CPU tests (tests/test_exact_div.py) share it.
//
// Everything here must give the bits of the operation it replaces: the frame is compared byte for
// byte with the CPU restatement.  None of it is taken on trust -- each form is used only for
// operands the host has checked one by one (rg_recip_div_ok) or whose range it has bounded
// (rg_camera_unscaled_ok).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define RG_EXACT_FN __host__ __device__ inline
#else
#define RG_EXACT_FN inline
#endif

// a / n from inv = 1.0 / n: one multiply and a residual correction, three instructions for the
// 30-odd of the IEEE f64 division expansion.  q0 = a * inv is off by at most an ulp; the first fma
// gives its residual a - q0 * n exactly, the second adds the residual's quotient.  Not correctly
// rounded for every (a, n) -- which is why a launch uses it only for the pairs rg_recip_div_ok
// has compared with the division.  The fmas are explicit: -ffp-contract=off leaves them alone.
RG_EXACT_FN double rg_recip_quot(double a, double n, double inv) {
    const double q0 = a * inv;
    return __builtin_fma(__builtin_fma(-q0, n, a), inv, q0);
}

// The dividends of the camera ray (ray.rs:46-51): pixel centres i + 0.5, i < n.
RG_EXACT_FN double rg_pixel_centre(uint32_t i) { return (double)i + 0.5; }

// Does rg_recip_quot(i + 0.5, n, inv) equal (i + 0.5) / n, bit for bit, for EVERY i < n -- and is inv
// the correctly rounded 1.0 / n, the only reciprocal the form is meant for?  (The residual step
// absorbs most of a reciprocal's last-bit error, so the sweep alone would pass many a wrong inv.)
// n divisions: 4 us for a 4K frame's width, cached per frame size by the launch context.
inline bool rg_recip_div_ok(uint32_t n, double inv) {
    if (n == 0) return false;
    const double nd = (double)n;
    if (!(inv == 1.0 / nd)) return false;
    for (uint32_t i = 0; i < n; ++i) {
        const double a = rg_pixel_centre(i);
        if (!(rg_recip_quot(a, nd, inv) == a / nd)) return false;
    }
    return true;
}
inline bool rg_recip_div_ok(uint32_t n) { return n != 0 && rg_recip_div_ok(n, 1.0 / (double)n); }

// Unsigned 32-bit division by a divisor known before the launch (Granlund & Montgomery 1994,
// figure 4.1): with l = ceil(log2 d), m = floor(2^32 (2^l - d) / d) + 1, t = mulhi(m, n),
// n / d = (t + ((n - t) >> min(l, 1))) >> max(l - 1, 0) for EVERY n < 2^32 and 1 <= d < 2^32 --
// a multiply-high, a subtraction, an addition and two shifts for the 25-odd instructions of the
// f32-reciprocal expansion.  sh packs the two shift counts: sh1 | sh2 << 8.
struct RgMagicU32 {
    uint32_t m, sh;
};
inline RgMagicU32 rg_magic_u32(uint32_t d) {  // d >= 1
    uint32_t l = 0;
    while (l < 32 && ((uint64_t)1 << l) < d) ++l;
    const uint64_t m = ((((uint64_t)1 << l) - d) << 32) / d + 1;  // < 2^32: (2^l - d) / d < 1
    return RgMagicU32{(uint32_t)m, (l < 1 ? l : 1u) | ((l > 1 ? l - 1 : 0u) << 8)};
}
RG_EXACT_FN uint32_t rg_magic_div(uint32_t n, uint32_t m, uint32_t sh) {
    const uint32_t t = (uint32_t)(((uint64_t)m * n) >> 32);
    return (t + ((n - t) >> (sh & 0xffu))) >> (sh >> 8);
}

// material.rs:70-79 on a texture dimension: w % max with the sign of w (Rust's and C's %), then
// + max below zero -- i.e. w mod max in [0, max).  On |w| as a u32 (so i32::MIN is 2^31, no
// overflow), with the dimension's magic: r = |w| - (|w| / max) max, and a negative w maps to
// max - r, or to 0 where r is 0.  max >= 1.
RG_EXACT_FN uint32_t rg_wrap_i32(int32_t w, uint32_t max, uint32_t m, uint32_t sh) {
    const uint32_t aw = w < 0 ? 0u - (uint32_t)w : (uint32_t)w;
    const uint32_t r = aw - rg_magic_div(aw, m, sh) * max;
    return (w < 0 && r != 0u) ? max - r : r;
}

// A plane's texture axes (bodies.rs:155-169; rg_k_shade.h texture_coords): x = n x (0,0,1), or
// n x (0,1,0) where that is the zero vector; y = n x x.  They depend on the normal alone, so the host
// makes them once per plane -- with the kernel's very expressions, every product and difference
// rounded on its own (the library is built unfused), multiplications by the literal 0 and 1 and
// the signed zeros they leave included.
inline void rg_cross3(const double a[3], const double b[3], double out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}
inline void rg_plane_axes(const double n[3], double xa[3], double ya[3]) {
    const double ez[3] = {0.0, 0.0, 1.0}, ey[3] = {0.0, 1.0, 0.0};
    rg_cross3(n, ez, xa);
    if ((xa[0] * xa[0] + xa[1] * xa[1]) + xa[2] * xa[2] == 0.0) rg_cross3(n, ey, xa);
    rg_cross3(n, xa, ya);
}

// The camera ray's length is sqrt(s), s = (sx^2 + sy^2) + 1 with |sx| <= aspect * fov_adjustment and
// |sy| <= fov_adjustment (ray.rs:46-54; |2 q - 1| <= 1 for a quotient q in [0, 1]).  s >= 1 whatever
// the rounding (a sum of non-negative terms and 1), and s <= (1 + fa^2 (1 + aspect^2)) (1 + 2^-50).
// The f64 sqrt and division expansions rescale only operands far outside that:
//   * sqrt scales its operand up below 2^-767 and patches 0 and +inf;
//   * the division 1.0 / m scales when the divisor's exponent is within ~2 of the format's ends or
//     below 2^-1022 + 53, or the quotient's is; it patches NaN, 0, inf and denormal quotients.
// With s in [1, 2^100], m = sqrt(s) lies in [1, 2^50] and 1 / m in [2^-50, 1]: more than 700 binades
// from every one of those thresholds, so each scale factor is 1, each select takes the unpatched
// value, and the expansions without them (rg_k_math.h sqrt_unscaled / rcp_unscaled) give the same
// bits.  2^100 is no limit of the method, just far more than a camera needs (fov 179.9 degrees at
// an aspect of 4096 : 1 gives s ~ 2^44) and far less than the thresholds.  A NaN fails the test.
//
// The same expansions without their scaling, for operands only the LANE knows (rg_k_math.h
// sqrt_guarded / rcp_guarded / div_guarded): the admission is a test of the operand's exponent field.
// What the instructions and hipcc's expansions do outside the plain path, by their documentation:
//   * sqrt: ldexp(x, 256) in front and ldexp(., -128) behind where x < 2^-767; x itself for 0 and +inf
//     (v_cmp_class); a negative operand or a NaN goes through v_rsq_f64 to NaN;
//   * v_div_scale_f64 scales (by 2^+-128) where the denominator is denormal or its reciprocal would be
//     (biased exponent 0 or >= 2045), where the numerator's exponent is <= 53, where exponent(num) -
//     exponent(den) >= 768, or where the quotient would be denormal (difference <= -1023); v_div_fmas_f64
//     applies the scale only where v_div_scale said so; v_div_fixup_f64 replaces the value for a NaN,
//     zero or infinite operand and for quotients under- or overflowing, else copies it with the sign of
//     num ^ den, which the fma chain's nonzero result has already.
// With every operand's biased exponent in [RG_UNSCALED_EXP_LO, RG_UNSCALED_EXP_HI] = [767, 1279] (1023
// +- 256: |x| in [2^-256, 2^257)) none of that applies: x >= 2^-256 > 2^-767; exponents are > 53 and
// < 2045; two of them differ by at most 512 < 768, so a quotient lies in (2^-513, 2^514): normal; every
// intermediate of the refinement (the reciprocal, residuals of relative size >= 2^-108 or exactly 0) is
// normal or zero.  sqrt of an admitted x has its exponent in [-128, 128]: admitted as a divisor, so one
// test covers 1.0 / sqrt(x).  +-256 binades are no limit of the method (the nearest threshold, the
// numerator's exponent <= 53, is 714 binades below the window): they cover what a scene with
// coordinates below 1e100 that is worth the fast path produces, in one unsigned compare on the high
// dword -- which 0, denormals, inf, NaN, the far ends and (for sqrt, where the sign bit is part of
// the compared field) negative operands all fail.
#define RG_UNSCALED_EXP_LO 767u
#define RG_UNSCALED_EXP_HI 1279u
// hi: the operand's high dword.  sqrt's admission: a set sign bit fails.
RG_EXACT_FN bool rg_unscaled_ok_hi(uint32_t hi) {
    return hi - (RG_UNSCALED_EXP_LO << 20) < ((RG_UNSCALED_EXP_HI - RG_UNSCALED_EXP_LO + 1u) << 20);
}
// a division's operand: either sign
RG_EXACT_FN bool rg_unscaled_ok_abs_hi(uint32_t hi) { return rg_unscaled_ok_hi(hi & 0x7fffffffu); }
inline uint32_t rg_high_dword(double x) {
    uint64_t b;
    memcpy(&b, &x, sizeof b);
    return (uint32_t)(b >> 32);
}

#define RG_CAMERA_S_MAX 1.2676506002282294e30  // 2^100
inline bool rg_camera_unscaled_ok(double fov_adjustment, double aspect) {
    const double s = 1.0 + (fov_adjustment * fov_adjustment) * (1.0 + aspect * aspect);
    return s >= 1.0 && s <= RG_CAMERA_S_MAX;
}
