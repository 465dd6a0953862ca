// rg_bands.hip — the band-delivery engine behind the host-visible frames (rg_capi.hip)
// and the supersampled ones (rg_aa.hip), declared in rg_bands.h: a 4K RGBA8 frame is
// 33 MB, about as long on PCIe (~55 GB/s) as its render, so a frame is rendered in row
// bands on two render streams and band b's device-to-host copy (on a copy stream) runs
// while bands b+1.. render.  A pinned caller buffer (hipHostMalloc'd, or registered with
// rg_host_register) receives the DMA directly; a pageable one is fed from a ring of
// pinned staging slots by host memcpy (rg_copy_pool.cpp), overlapped with the following
// bands' DMA.  The callers enqueue the bands themselves, between rg_bands_fork and
// rg_bands_join.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "rg_bands.h"
#include "rg_internal.h"

#define RG_FRAME_SLACK 16  // bytes past the device frame

rg_status rg_bands_ensure(rg_band_res &r, int device, uint32_t bands, bool rs1_own_queue) {
    if (!r.cs) {
        bool good = ok(hipStreamCreateWithFlags(&r.rs[0], hipStreamNonBlocking));
        if (rs1_own_queue) {
            int cus = 0;
            (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
            std::vector<uint32_t> mask((size_t)std::max(1, (cus + 31) / 32), 0xFFFFFFFFu);
            if (cus % 32) mask.back() = (1u << (cus % 32)) - 1u;
            good = good && ok(hipExtStreamCreateWithCUMask(&r.rs[1], (uint32_t)mask.size(), mask.data()));
        } else {
            good = good && ok(hipStreamCreateWithFlags(&r.rs[1], hipStreamNonBlocking));
        }
        good = good && ok(hipStreamCreateWithFlags(&r.cs, hipStreamNonBlocking));
        good = good && ok(hipEventCreate(&r.ev_t0)) && ok(hipEventCreate(&r.ev_t1)) &&
               ok(hipEventCreateWithFlags(&r.ev_join, hipEventDisableTiming));
        if (!good) {
            rg_bands_release(r);
            return RG_ERR_DEVICE;
        }
    }
    for (std::vector<hipEvent_t> *v : {&r.ev_done, &r.ev_copy})
        while (v->size() < bands) {
            hipEvent_t e = nullptr;
            if (!ok(hipEventCreateWithFlags(&e, hipEventDisableTiming))) return RG_ERR_DEVICE;
            v->push_back(e);
        }
    return rg_grow(RG_MEM_PINNED, r.h_snap, r.h_snap_cap, (size_t)bands * 4 * sizeof(unsigned long long));
}

void rg_bands_release(rg_band_res &r) {
    for (hipStream_t st : {r.rs[0], r.rs[1], r.cs})
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    for (hipEvent_t e : r.ev_done) (void)hipEventDestroy(e);
    for (hipEvent_t e : r.ev_copy) (void)hipEventDestroy(e);
    for (hipEvent_t e : {r.ev_t0, r.ev_t1, r.ev_join})
        if (e) (void)hipEventDestroy(e);
    if (r.d_rgba) (void)hipFree(r.d_rgba);
    if (r.d_rgb) (void)hipFree(r.d_rgb);
    if (r.h_stage) (void)hipHostFree(r.h_stage);
    if (r.h_snap) (void)hipHostFree(r.h_snap);
    r = rg_band_res{};
}

rg_status rg_bands_ensure_frame(rg_band_res &r, size_t px, bool want_rgb) {
    const rg_status st = rg_grow(RG_MEM_DEVICE, r.d_rgba, r.d_rgba_cap, px * 4 + RG_FRAME_SLACK);
    if (st != RG_OK || !want_rgb) return st;
    return rg_grow(RG_MEM_DEVICE, r.d_rgb, r.d_rgb_cap, px * 12 + RG_FRAME_SLACK);
}

rg_status rg_bands_drain(rg_band_res &r, rg_status status) {
    (void)hipStreamSynchronize(r.rs[1]);
    (void)hipStreamSynchronize(r.rs[0]);
    (void)hipStreamSynchronize(r.cs);
    (void)hipGetLastError();
    return status;
}

rg_copy_pool &rg_bands_pool(rg_band_res &r) {
    if (!r.pool) r.pool = std::make_shared<rg_copy_pool>(RG_COPY_HELPERS);
    return *r.pool;
}

bool rg_bands_fork(rg_band_res &r) {
    return ok(hipEventRecord(r.ev_t0, r.rs[0])) && ok(hipStreamWaitEvent(r.rs[1], r.ev_t0, 0));
}

bool rg_bands_join(rg_band_res &r) {
    return ok(hipEventRecord(r.ev_join, r.rs[1])) && ok(hipStreamWaitEvent(r.rs[0], r.ev_join, 0)) &&
           ok(hipEventRecord(r.ev_t1, r.rs[0]));
}

rg_status rg_bands_deliver(rg_band_res &r, const rg_band_plan &p, const uint8_t *d_rgba, const float *d_rgb,
                           uint8_t *rgba_out, float *rgb_out) {
    const bool want_rgb = rgb_out != nullptr;
    const size_t row4 = (size_t)p.width * 4, row12 = (size_t)p.width * 12, W3 = (size_t)p.width * 3;
    // the route: straight into a page-locked destination, else through the staging ring (grown
    // here, with the bands already rendering: the ring is idle between calls)
    const bool direct = rg_host_is_pinned(rgba_out, (size_t)p.host_rows * row4) &&
                        (!want_rgb || rg_host_is_pinned(rgb_out, (size_t)p.host_rows * row12));
    const uint32_t R = RG_IMAGE_STAGE_SLOTS;
    const size_t slot_bytes = (size_t)p.band_rows * (row4 + (want_rgb ? row12 : 0));
    if (!direct) {
        const rg_status st = rg_grow(RG_MEM_PINNED, r.h_stage, r.h_stage_cap, (size_t)R * slot_bytes);
        if (st != RG_OK) return rg_bands_drain(r, st);
    }
    auto stage_rgba = [&](uint32_t b) { return static_cast<uint8_t *>(r.h_stage) + (size_t)(b % R) * slot_bytes; };
    auto stage_rgb = [&](uint32_t b) { return reinterpret_cast<float *>(stage_rgba(b) + (size_t)p.band_rows * row4); };
    // band b's finished rows to the caller (or its staging slot) behind the band's event
    auto enqueue_copy = [&](uint32_t b) -> bool {
        const size_t off = (size_t)b * p.band_rows;
        const size_t n = rg_band_rows(p, b);
        uint8_t *dst4 = direct ? rgba_out + off * row4 : stage_rgba(b);
        float *dst12 = want_rgb ? (direct ? rgb_out + off * W3 : stage_rgb(b)) : nullptr;
        if (!ok(hipStreamWaitEvent(r.cs, r.ev_done[b], 0)) ||
            !ok(hipMemcpyAsync(dst4, d_rgba + off * row4, n * row4, hipMemcpyDeviceToHost, r.cs)))
            return false;
        if (dst12 && !ok(hipMemcpyAsync(dst12, d_rgb + off * W3, n * row12, hipMemcpyDeviceToHost, r.cs))) return false;
        return ok(hipEventRecord(r.ev_copy[b], r.cs));
    };
    if (direct) {
        for (uint32_t b = 0; b < p.bands; ++b)
            if (!enqueue_copy(b)) return rg_bands_drain(r, RG_ERR_DEVICE);
        if (!ok(hipStreamSynchronize(r.cs))) return rg_bands_drain(r, RG_ERR_DEVICE);
    } else {
        // pageable destination: DMA into the pinned staging ring, then a parallel host copy of
        // each band while the next bands' DMA runs
        rg_copy_pool &pool = rg_bands_pool(r);
        rg_copy_pool::Active active(pool);
        for (uint32_t b = 0; b < std::min(p.bands, R); ++b)
            if (!enqueue_copy(b)) return rg_bands_drain(r, RG_ERR_DEVICE);
        for (uint32_t b = 0; b < p.bands; ++b) {
            if (!ok(hipEventSynchronize(r.ev_copy[b]))) return rg_bands_drain(r, RG_ERR_DEVICE);
            const size_t off = (size_t)b * p.band_rows;
            const size_t n = rg_band_rows(p, b);
            pool.copy(rgba_out + off * row4, stage_rgba(b), n * row4);
            if (want_rgb) pool.copy(rgb_out + off * W3, stage_rgb(b), n * row12);
            if (b + R < p.bands && !enqueue_copy(b + R)) return rg_bands_drain(r, RG_ERR_DEVICE);
        }
    }
    if (!ok(hipStreamSynchronize(r.rs[0])) || !ok(hipStreamSynchronize(r.rs[1]))) return rg_bands_drain(r, RG_ERR_DEVICE);
    return RG_OK;
}

// Bands in ascending pixel order, so "the lowest failing pixel" is the first failing band (rg_stats_merge.h).
static rg_status rg_merge_band_snaps(const unsigned long long *snap, int n, rg_stats *total) {
    std::memset(total, 0, sizeof *total);
    total->error_pixel = -1;
    rg_status err = RG_OK;
    for (int b = 0; b < n; ++b) {
        rg_stats bs;
        const rg_status e = rg_snap_status(snap + 4 * b, &bs);
        rg_stats_add(*total, err, bs, e);
    }
    return err;
}

rg_status rg_finish_stats(const unsigned long long *snap, int n, hipEvent_t ev_t0, hipEvent_t ev_t1, rg_stats *stats) {
    rg_stats total;
    const rg_status err = rg_merge_band_snaps(snap, n, &total);
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, ev_t0, ev_t1);
    total.kernel_ms = ms;
    if (stats) *stats = total;
    return err;
}
