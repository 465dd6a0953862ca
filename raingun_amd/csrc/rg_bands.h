// rg_bands.h — a frame rendered in row bands on two alternating render streams and
// delivered to the caller band by band: the streams, events and buffers of that
// (rg_band_res), the fork and join of the two streams, the delivery and the stats tail.
// Used by the host-visible frames (rg_capi.hip) and the supersampled ones (rg_aa.hip),
// each with an instance of its own; implemented in rg_bands.hip.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <memory>
#include <vector>

#include "../../include/raingun.h"
#include "rg_band_plan.h"
#include "rg_copy_pool.h"

#define RG_IMAGE_STAGE_SLOTS 4  // pinned staging slots of a pageable destination

struct rg_band_res {
    std::shared_ptr<rg_copy_pool> pool;      // pageable destinations (rg_bands_pool)
    hipStream_t rs[2] = {nullptr, nullptr};  // render streams (bands alternate)
    hipStream_t cs = nullptr;                // device-to-host copies
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr, ev_join = nullptr;
    std::vector<hipEvent_t> ev_done, ev_copy;  // per band: rendered, copied
    void *d_rgba = nullptr;                    // the frame in device memory
    size_t d_rgba_cap = 0;
    void *d_rgb = nullptr;
    size_t d_rgb_cap = 0;
    void *h_stage = nullptr;  // pinned staging ring
    size_t h_stage_cap = 0;
    unsigned long long *h_snap = nullptr;  // pinned: 4 counter words per band
    size_t h_snap_cap = 0;                 // bytes
};

#pragma GCC visibility push(hidden)

// Streams (rs[0], rs[1], cs, in this order) and timing events on first use; band events and
// counter snapshots for `bands` bands.  rs1_own_queue: rs[1] is a CU-masked stream (every CU),
// which gets a hardware queue of its own.
rg_status rg_bands_ensure(rg_band_res &r, int device, uint32_t bands, bool rs1_own_queue);
void rg_bands_release(rg_band_res &r);
// The device frame of `px` pixels (d_rgba; want_rgb: d_rgb too).
rg_status rg_bands_ensure_frame(rg_band_res &r, size_t px, bool want_rgb);
// Wait for everything on rs[1], rs[0] and cs, clear the runtime's error, return `status`.  Once
// a kernel or a DMA that stores into the caller's buffer is enqueued, every error exit goes
// through here: the caller owns its buffer again when the call returns (rendering.rs:24-38
// returns a finished ImageBuffer).
rg_status rg_bands_drain(rg_band_res &r, rg_status status);
rg_copy_pool &rg_bands_pool(rg_band_res &r);  // created on first use

// ev_t0 on rs[0], rs[1] behind it / rs[0] behind rs[1], ev_t1 on rs[0].
bool rg_bands_fork(rg_band_res &r);
bool rg_bands_join(rg_band_res &r);

// After the join: band b of plan `p` (rows [b band_rows, ..) of the device frame d_rgba / d_rgb)
// goes to the same rows of rgba_out / rgb_out (nullable, with d_rgb) on cs behind ev_done[b]: by
// DMA into page-locked destinations, else through the staging ring and the copy pool.  Returns
// with all three streams idle, on failure through rg_bands_drain.
rg_status rg_bands_deliver(rg_band_res &r, const rg_band_plan &p, const uint8_t *d_rgba, const float *d_rgb,
                           uint8_t *rgba_out, float *rgb_out);

// Ray counts summed over n band snapshots (4 words each), the status and pixel of the lowest
// erroring pixel (rg_stats_merge.h; bands come in row order, so it is the first erroring
// snapshot's), kernel_ms = ev_t0 .. ev_t1, into `stats` (nullable).
rg_status rg_finish_stats(const unsigned long long *snap, int n, hipEvent_t ev_t0, hipEvent_t ev_t1, rg_stats *stats);

#pragma GCC visibility pop
