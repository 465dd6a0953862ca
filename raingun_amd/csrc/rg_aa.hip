// rg_aa.hip — supersampled anti-aliasing: samples x samples rays per pixel on the
// regular sub-pixel grid, box-filtered (rg_render_image_aa, rg_render_aa_async,
// rg_resolve_box, rg_debug_set_aa_band_rows).
//
// Ray::create_prime (ray.rs:43-49) puts pixel (x, y)'s sample at ((x + 0.5) / width,
// (y + 0.5) / height) with aspect = width / height, so the k W x k H frame has its
// samples exactly on the k x k sub-pixel grid of the W x H frame: the supersampled
// frame is the existing render kernel at k W x k H (rg_launch_tiles, untouched) plus
// a resolve (rg_resolve.hip).  The frame is cut into bands of Rb output rows; band b
// renders, as tile b of the tiling {k Rb, bands, b}, into a scratch slot (RGBA8,
// which the render kernel always writes, and f32 RGB: 16 B per sample) and is
// resolved on the same stream into the W x H result.  Bands alternate between two
// streams with a slot each, so a band's resolve overlaps the next band's render and a
// slot's reuse is ordered by its stream.  The host entry copies each band's finished
// rows to the caller on a copy stream behind an event, as rg_render_host does.  No
// exception or abort crosses the ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/raingun.h"
#include "../../include/raingun_debug.h"
#include "rg_device.h"
#include "rg_internal.h"
#include "rg_launchers.h"

#pragma clang fp contract(off)

void rg_aa_res_release(rg_aa_res &r) {
    for (hipStream_t &st : r.rs)
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); st = nullptr; }
    if (r.cs) { (void)hipStreamSynchronize(r.cs); (void)hipStreamDestroy(r.cs); r.cs = nullptr; }
    for (hipEvent_t e : r.ev_done) (void)hipEventDestroy(e);
    for (hipEvent_t e : r.ev_copy) (void)hipEventDestroy(e);
    for (hipEvent_t *e : {&r.ev_t0, &r.ev_t1, &r.ev_join, &r.ev_fork})
        if (*e) { (void)hipEventDestroy(*e); *e = nullptr; }
    for (int i = 0; i < 2; ++i) {
        if (r.slot_rgba[i]) (void)hipFree(r.slot_rgba[i]);
        if (r.slot_rgb[i]) (void)hipFree(r.slot_rgb[i]);
    }
    if (r.d_rgba) (void)hipFree(r.d_rgba);
    if (r.d_rgb) (void)hipFree(r.d_rgb);
    if (r.h_stage) (void)hipHostFree(r.h_stage);
    if (r.h_snap) (void)hipHostFree(r.h_snap);
    r = rg_aa_res{};
}

namespace {

// A validated supersampled frame: W x H output pixels, k x k samples each, nb bands of Rb output rows.
struct aa_plan {
    uint32_t W, H, k, Rb, nb;
};

// The first failing check decides the status; no HIP call.
rg_status aa_validate(const void *scene, uint32_t W, uint32_t H, uint32_t k, const void *rgba) {
    if (!scene || !rgba || W == 0 || H == 0 || k < 1 || k > RG_AA_MAX_SAMPLES) return RG_ERR_INVALID_ARGUMENT;
    if ((unsigned long long)k * W * ((unsigned long long)k * H) >= (1ull << 32))
        return RG_ERR_INVALID_ARGUMENT;  // the sample frame keeps the reference's u32 pixel index (rendering.rs:27)
    if (W < H) return RG_ERR_PORTRAIT;   // ray.rs:42
    return RG_OK;
}

// Output rows per band: one slot (k Rb rows of k W samples, 16 B each) within RG_AA_SLOT_BYTES,
// whole 8-row tile rows, at least RG_AA_MIN_BAND_ROWS; rg_debug_set_aa_band_rows overrides.
aa_plan aa_make_plan(const rg_scene *s, uint32_t W, uint32_t H, uint32_t k) {
    uint32_t rb;
    if (s->aa_band_rows > 0) {
        rb = (uint32_t)s->aa_band_rows;
    } else {
        const size_t per_row = (size_t)k * k * W * 16;
        rb = (uint32_t)std::min<size_t>(RG_AA_SLOT_BYTES / per_row, 0x10000u) & ~7u;
        rb = std::max<uint32_t>(rb, RG_AA_MIN_BAND_ROWS);
    }
    rb = std::min(rb, H);
    return {W, H, k, rb, (H + rb - 1) / rb};
}

bool ensure_events(std::vector<hipEvent_t> &v, size_t n) {
    while (v.size() < n) {
        hipEvent_t e = nullptr;
        if (!ok(hipEventCreateWithFlags(&e, hipEventDisableTiming))) return false;
        v.push_back(e);
    }
    return true;
}

// Streams and events on first use; the slots, the band events and (snaps) the counter snapshots
// for this plan.
rg_status ensure_aa_res(const rg_scene *s, const aa_plan &p, bool snaps) {
    rg_aa_res &r = s->aa;
    if (!r.cs) {
        bool good = true;
        for (hipStream_t &st : r.rs) good = good && ok(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        good = good && ok(hipStreamCreateWithFlags(&r.cs, hipStreamNonBlocking));
        good = good && ok(hipEventCreate(&r.ev_t0)) && ok(hipEventCreate(&r.ev_t1)) &&
               ok(hipEventCreateWithFlags(&r.ev_join, hipEventDisableTiming)) &&
               ok(hipEventCreateWithFlags(&r.ev_fork, hipEventDisableTiming));
        if (!good) {
            rg_aa_res_release(r);
            return RG_ERR_DEVICE;
        }
    }
    if (!ensure_events(r.ev_done, p.nb) || !ensure_events(r.ev_copy, p.nb)) return RG_ERR_DEVICE;
    const size_t samples = (size_t)p.k * p.Rb * p.k * p.W;
    rg_status st = RG_OK;
    for (int i = 0; i < (p.nb > 1 ? 2 : 1); ++i)
        if ((st = rg_grow(RG_MEM_DEVICE, r.slot_cap[i], samples,
                          {{r.slot_rgba[i], samples * 4 + 16}, {r.slot_rgb[i], samples * 12 + 16}})) != RG_OK)
            return st;
    if (snaps && (st = rg_grow(RG_MEM_PINNED, r.h_snap, r.h_snap_cap, (size_t)p.nb * 4 * sizeof(unsigned long long))) != RG_OK)
        return st;
    return RG_OK;
}

// Output rows of band b.
uint32_t band_out_rows(const aa_plan &p, uint32_t b) {
    const uint32_t r0 = b * p.Rb;
    return std::min(p.H, r0 + p.Rb) - r0;
}

// Every band's render and resolve, bands alternating between the two streams; out_rgba / out_rgb
// (nullable): the W x H result in device memory.  ev_done[b]: band b's rows are resolved.
rg_status enqueue_bands(const rg_scene *s, const aa_plan &p, uint8_t *out_rgba, float *out_rgb, bool snaps) {
    rg_aa_res &r = s->aa;
    for (uint32_t b = 0; b < p.nb; ++b) {
        const int i = (int)(b & 1u);
        hipStream_t rs = r.rs[i];
        rg_launch_desc d;
        d.width = p.k * p.W;
        d.height = p.k * p.H;
        d.tiling = rg_tiling{p.k * p.Rb, p.nb, b};  // exactly sample rows [b k Rb, (b + 1) k Rb)
        d.rgba = static_cast<uint8_t *>(r.slot_rgba[i]);
        d.rgb = static_cast<float *>(r.slot_rgb[i]);
        d.stream = rs;
        d.snap = snaps ? r.h_snap + 4 * (size_t)b : nullptr;
        const rg_status st = rg_launch_tiles(s, d);
        if (st != RG_OK) return st;
        const size_t off = (size_t)b * p.Rb * p.W;  // the last band is partial: only rows below H
        if (!ok(rg_launch_resolve(d.rgb, p.W, band_out_rows(p, b), p.k, out_rgba + off * 4,
                                  out_rgb ? out_rgb + off * 3 : nullptr, rs)) ||
            !ok(hipEventRecord(r.ev_done[b], rs)))
            return RG_ERR_DEVICE;
    }
    return RG_OK;
}

// Rays summed over the bands; a device error names the OUTPUT pixel that contains the
// lowest-index failing sample of the k W x k H frame.
rg_status aa_stats(const rg_scene *s, const aa_plan &p, rg_stats *stats) {
    rg_aa_res &r = s->aa;
    rg_stats total;
    const rg_status err = rg_merge_band_snaps(r.h_snap, (int)p.nb, &total);
    if (err != RG_OK) {
        const uint32_t e = (uint32_t)total.error_pixel, kw = p.k * p.W;
        total.error_pixel = (int32_t)((e / kw / p.k) * p.W + (e % kw) / p.k);
    }
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, r.ev_t0, r.ev_t1);  // first render .. last resolve
    total.kernel_ms = ms;
    if (stats) *stats = total;
    return err;
}

rg_status drain(rg_aa_res &r, rg_status e) {
    (void)hipStreamSynchronize(r.rs[0]);
    (void)hipStreamSynchronize(r.rs[1]);
    (void)hipStreamSynchronize(r.cs);
    (void)hipGetLastError();
    return e;
}

rg_status render_aa_host(const rg_scene *s, const aa_plan &p, uint8_t *rgba_out, float *rgb_out, rg_stats *stats) {
    rg_aa_res &r = s->aa;
    rg_status st = ensure_aa_res(s, p, true);
    if (st != RG_OK) return st;
    const bool want_rgb = rgb_out != nullptr;
    const size_t row4 = (size_t)p.W * 4, row12 = (size_t)p.W * 12;
    if ((st = rg_grow(RG_MEM_DEVICE, r.d_rgba, r.d_rgba_cap, (size_t)p.H * row4 + 16)) != RG_OK) return st;
    if (want_rgb && (st = rg_grow(RG_MEM_DEVICE, r.d_rgb, r.d_rgb_cap, (size_t)p.H * row12 + 16)) != RG_OK) return st;
    const bool direct = rg_host_is_pinned(rgba_out, (size_t)p.H * row4) &&
                        (!want_rgb || rg_host_is_pinned(rgb_out, (size_t)p.H * row12));
    const uint32_t R = RG_IMAGE_STAGE_SLOTS;
    const size_t slot_bytes = (size_t)p.Rb * (row4 + (want_rgb ? row12 : 0));
    if (!direct && (st = rg_grow(RG_MEM_PINNED, r.h_stage, r.h_stage_cap, (size_t)R * slot_bytes)) != RG_OK) return st;
    auto stage_rgba = [&](uint32_t b) { return static_cast<uint8_t *>(r.h_stage) + (size_t)(b % R) * slot_bytes; };
    auto stage_rgb = [&](uint32_t b) { return reinterpret_cast<float *>(stage_rgba(b) + (size_t)p.Rb * row4); };
    uint8_t *d_rgba = static_cast<uint8_t *>(r.d_rgba);
    float *d_rgb = want_rgb ? static_cast<float *>(r.d_rgb) : nullptr;

    if (!ok(hipEventRecord(r.ev_t0, r.rs[0])) || !ok(hipStreamWaitEvent(r.rs[1], r.ev_t0, 0))) return RG_ERR_DEVICE;
    if ((st = enqueue_bands(s, p, d_rgba, d_rgb, true)) != RG_OK) return drain(r, st);
    if (!ok(hipEventRecord(r.ev_join, r.rs[1])) || !ok(hipStreamWaitEvent(r.rs[0], r.ev_join, 0)) ||
        !ok(hipEventRecord(r.ev_t1, r.rs[0])))
        return drain(r, RG_ERR_DEVICE);
    // band b's finished rows to the caller (or its staging slot) behind the band's event
    auto enqueue_copy = [&](uint32_t b) -> bool {
        const size_t off = (size_t)b * p.Rb;
        const uint32_t n = band_out_rows(p, b);
        uint8_t *dst4 = direct ? rgba_out + off * row4 : stage_rgba(b);
        float *dst12 = want_rgb ? (direct ? rgb_out + off * (size_t)p.W * 3 : stage_rgb(b)) : nullptr;
        if (!ok(hipStreamWaitEvent(r.cs, r.ev_done[b], 0)) ||
            !ok(hipMemcpyAsync(dst4, d_rgba + off * row4, (size_t)n * row4, hipMemcpyDeviceToHost, r.cs)))
            return false;
        if (dst12 && !ok(hipMemcpyAsync(dst12, d_rgb + off * (size_t)p.W * 3, (size_t)n * row12, hipMemcpyDeviceToHost, r.cs)))
            return false;
        return ok(hipEventRecord(r.ev_copy[b], r.cs));
    };
    if (direct) {
        for (uint32_t b = 0; b < p.nb; ++b)
            if (!enqueue_copy(b)) return drain(r, RG_ERR_DEVICE);
        if (!ok(hipStreamSynchronize(r.cs))) return drain(r, RG_ERR_DEVICE);
    } else {
        // pageable destination: DMA into the pinned staging ring, then a parallel host copy of
        // each band while the next bands' DMA runs
        if (!r.pool) r.pool = std::make_shared<rg_copy_pool>(RG_COPY_HELPERS);
        rg_copy_pool::Active active(*r.pool);
        for (uint32_t b = 0; b < std::min(p.nb, R); ++b)
            if (!enqueue_copy(b)) return drain(r, RG_ERR_DEVICE);
        for (uint32_t b = 0; b < p.nb; ++b) {
            if (!ok(hipEventSynchronize(r.ev_copy[b]))) return drain(r, RG_ERR_DEVICE);
            const size_t off = (size_t)b * p.Rb;
            const uint32_t n = band_out_rows(p, b);
            r.pool->copy(rgba_out + off * row4, stage_rgba(b), (size_t)n * row4);
            if (want_rgb) r.pool->copy(rgb_out + off * (size_t)p.W * 3, stage_rgb(b), (size_t)n * row12);
            if (b + R < p.nb && !enqueue_copy(b + R)) return drain(r, RG_ERR_DEVICE);
        }
    }
    if (!ok(hipStreamSynchronize(r.rs[0])) || !ok(hipStreamSynchronize(r.rs[1]))) return drain(r, RG_ERR_DEVICE);
    return aa_stats(s, p, stats);
}

}  // namespace

extern "C" {

rg_status rg_render_image_aa(const rg_scene *s, uint32_t width, uint32_t height, uint32_t samples, uint8_t *rgba_out,
                             float *rgb_out, rg_stats *stats) {
    const rg_status v = aa_validate(s, width, height, samples, rgba_out);
    if (v != RG_OK) return v;
    if (samples == 1 && !rgb_out) return rg_render_image(s, width, height, rgba_out, stats);  // the same bytes
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    return render_aa_host(s, aa_make_plan(s, width, height, samples), rgba_out, rgb_out, stats);
}

rg_status rg_render_aa_async(const rg_scene *s, uint32_t width, uint32_t height, uint32_t samples, uint8_t *rgba_dev,
                             float *rgb_dev, void *stream, rg_stats *stats) {
    const rg_status v = aa_validate(s, width, height, samples, rgba_dev);
    if (v != RG_OK) return v;
    if (samples == 1 && !rgb_dev) {  // the same bytes
        const rg_tiling whole = {height, 1, 0};
        return rg_render_tiles_async(s, width, height, &whole, rgba_dev, nullptr, stream, stats);
    }
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    const aa_plan p = aa_make_plan(s, width, height, samples);
    const bool snaps = stats != nullptr;
    rg_status st = ensure_aa_res(s, p, snaps);
    if (st != RG_OK) return st;
    rg_aa_res &r = s->aa;
    hipStream_t caller = static_cast<hipStream_t>(stream);
    // the scene's two streams fork from the caller's stream and join it again
    if (!ok(hipEventRecord(r.ev_fork, caller)) || !ok(hipStreamWaitEvent(r.rs[0], r.ev_fork, 0)) ||
        !ok(hipStreamWaitEvent(r.rs[1], r.ev_fork, 0)) || !ok(hipEventRecord(r.ev_t0, r.rs[0])))
        return RG_ERR_DEVICE;
    st = enqueue_bands(s, p, rgba_dev, rgb_dev, snaps);
    const bool joined = ok(hipEventRecord(r.ev_join, r.rs[1])) && ok(hipStreamWaitEvent(r.rs[0], r.ev_join, 0)) &&
                        ok(hipEventRecord(r.ev_t1, r.rs[0])) && ok(hipStreamWaitEvent(caller, r.ev_t1, 0));
    if (st != RG_OK || !joined) return drain(r, st != RG_OK ? st : RG_ERR_DEVICE);
    if (!stats) return RG_OK;
    if (!ok(hipStreamSynchronize(caller))) return RG_ERR_DEVICE;
    return aa_stats(s, p, stats);
}

rg_status rg_resolve_box(int32_t device, const float *rgb_in, uint32_t width, uint32_t height, uint32_t samples,
                         uint8_t *rgba_out, float *rgb_out) {
    if (device < 0 || !rgb_in || !rgba_out || width == 0 || height == 0 || samples < 1 || samples > RG_AA_MAX_SAMPLES)
        return RG_ERR_INVALID_ARGUMENT;
    if ((unsigned long long)samples * width * ((unsigned long long)samples * height) >= (1ull << 32))
        return RG_ERR_INVALID_ARGUMENT;
    if (!ok(hipSetDevice(device))) return RG_ERR_DEVICE;
    const size_t in_bytes = (size_t)samples * width * samples * height * 12, px = (size_t)width * height;
    void *d_in = nullptr, *d_rgba = nullptr, *d_rgb = nullptr;
    rg_status st = RG_OK;
    if (!ok(hipMalloc(&d_in, in_bytes)) || !ok(hipMalloc(&d_rgba, px * 4)) || (rgb_out && !ok(hipMalloc(&d_rgb, px * 12)))) {
        (void)hipGetLastError();
        st = RG_ERR_OUT_OF_MEMORY;
    }
    if (st == RG_OK &&
        (!ok(hipMemcpy(d_in, rgb_in, in_bytes, hipMemcpyHostToDevice)) ||
         !ok(rg_launch_resolve(static_cast<const float *>(d_in), width, height, samples, static_cast<uint8_t *>(d_rgba),
                               static_cast<float *>(d_rgb), nullptr)) ||
         !ok(hipMemcpy(rgba_out, d_rgba, px * 4, hipMemcpyDeviceToHost)) ||
         (rgb_out && !ok(hipMemcpy(rgb_out, d_rgb, px * 12, hipMemcpyDeviceToHost)))))
        st = RG_ERR_DEVICE;
    if (d_in) (void)hipFree(d_in);
    if (d_rgba) (void)hipFree(d_rgba);
    if (d_rgb) (void)hipFree(d_rgb);
    return st;
}

rg_status rg_debug_set_aa_band_rows(rg_scene *s, int32_t rows) {
    if (!s || rows < 0) return RG_ERR_INVALID_ARGUMENT;
    s->aa_band_rows = rows;
    return RG_OK;
}

}  // extern "C"
