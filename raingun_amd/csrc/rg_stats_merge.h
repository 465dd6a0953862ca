// rg_stats_merge.h — which statuses still deliver a frame, and the one rule for merging the statistics of the
// passes (or bands) of a frame.  Pure arithmetic, no HIP: usable from a plain g++ program
// (tests/native/stats_merge_test.cpp).
#pragma once
#include <cstdint>

#include "../../include/raingun.h"

// A frame is delivered on RG_OK and on the reference's three panics (include/raingun.h).  Only
// rg_render_kernel.h has a site that raises RG_ERR_TRANSMISSION; the AOV and AO kernels never report it.
inline bool rg_delivers_frame(rg_status st) {
    return st == RG_OK || st == RG_ERR_AABB_NORMAL || st == RG_ERR_NAN_DISTANCE || st == RG_ERR_TRANSMISSION;
}

// Fold one pass into a frame's running total (start: rays zero, error_pixel -1, st RG_OK): the three ray
// counts add up; of the failing passes the one with the lower pixel index gives the status and the pixel, and
// on a tie `total` keeps what it holds, so the pass folded first wins.  Indices compare as the u32 they are
// (rg_snap_status narrows a sample frame's index, which may pass 2^31, to error_pixel's i32).  kernel_ms is
// the caller's business.
//
// The bands of a frame (rg_finish_stats) used to take "the first failing band".  A band's error key names the
// IMAGE pixel (y * width + x with the image row y, rg_render_kernel.h), and every caller's snapshots are in
// ascending pixel order: row bands b = 0, 1, .. of one frame (rg_render_host banded, the supersampled bands,
// whose skipped ones are zero), part A above part B of a split frame, or a single snapshot (a sharded tiling
// goes through rg_one_band: n == 1; the one-launch and streaming paths likewise).  So the first failing band is
// the one with the lowest pixel, and two bands never tie.
inline void rg_stats_add(rg_stats &total, rg_status &st, const rg_stats &pass, rg_status pass_st) {
    total.rays.primary += pass.rays.primary;
    total.rays.shadow += pass.rays.shadow;
    total.rays.secondary += pass.rays.secondary;
    if (pass_st != RG_OK && (st == RG_OK || (uint32_t)pass.error_pixel < (uint32_t)total.error_pixel)) {
        st = pass_st;
        total.error_pixel = pass.error_pixel;
    }
}
