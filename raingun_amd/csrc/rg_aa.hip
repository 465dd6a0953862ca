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
// slot's reuse is ordered by its stream.  The streams, the events, the delivery of each
// band's finished rows to the host entry's caller and the stats tail are rg_render_host's
// (rg_bands.hip), on an instance of the band resources of its own; the band arithmetic
// is in rg_band_plan.h.  No exception or abort crosses the ABI.
#include <hip/hip_runtime.h>

#include "../../include/raingun.h"
#include "../../include/raingun_debug.h"
#include "rg_device.h"
#include "rg_internal.h"
#include "rg_launchers.h"

#pragma clang fp contract(off)

void rg_aa_res_release(rg_aa_res &r) {
    rg_bands_release(r);  // first: it waits for the streams
    if (r.ev_fork) (void)hipEventDestroy(r.ev_fork);
    for (int i = 0; i < 2; ++i) {
        if (r.slot_rgba[i]) (void)hipFree(r.slot_rgba[i]);
        if (r.slot_rgb[i]) (void)hipFree(r.slot_rgb[i]);
    }
    r = rg_aa_res{};
}

namespace {

// A validated supersampled frame: width x host_rows output pixels in bands of band_rows rows,
// k x k samples each.
struct aa_plan : rg_band_plan {
    uint32_t k;
};

// The first failing check decides the status; no HIP call.
rg_status aa_validate(const void *scene, uint32_t W, uint32_t H, uint32_t k, const void *rgba) {
    if (!scene || !rgba || W == 0 || H == 0 || k < 1 || k > RG_AA_MAX_SAMPLES) return RG_ERR_INVALID_ARGUMENT;
    if ((unsigned long long)k * W * ((unsigned long long)k * H) >= (1ull << 32))
        return RG_ERR_INVALID_ARGUMENT;  // the sample frame keeps the reference's u32 pixel index (rendering.rs:27)
    if (W < H) return RG_ERR_PORTRAIT;   // ray.rs:42
    return RG_OK;
}

aa_plan aa_make_plan(const rg_scene *s, uint32_t W, uint32_t H, uint32_t k) {
    return {rg_aa_band_plan(s->aa_band_rows, W, H, k, RG_AA_SLOT_BYTES, RG_AA_MIN_BAND_ROWS), k};
}

// Streams and events (plain streams: the two render streams of this instance share the
// process's queues) and the sample slots for this plan.
rg_status ensure_aa_res(const rg_scene *s, const aa_plan &p) {
    rg_aa_res &r = s->aa;
    rg_status st = rg_bands_ensure(r, s->device, p.bands, false);
    if (st != RG_OK) return st;
    if (!r.ev_fork && !ok(hipEventCreateWithFlags(&r.ev_fork, hipEventDisableTiming))) return RG_ERR_DEVICE;
    const size_t samples = (size_t)p.k * p.band_rows * p.k * p.width;
    for (int i = 0; i < (p.bands > 1 ? 2 : 1); ++i)
        if ((st = rg_grow(RG_MEM_DEVICE, r.slot_cap[i], samples,
                          {{r.slot_rgba[i], samples * 4 + 16}, {r.slot_rgb[i], samples * 12 + 16}})) != RG_OK)
            return st;
    return RG_OK;
}

// Every band's render and resolve, bands alternating between the two streams; out_rgba / out_rgb
// (nullable): the W x H result in device memory.  ev_done[b]: band b's rows are resolved.
rg_status enqueue_bands(const rg_scene *s, const aa_plan &p, uint8_t *out_rgba, float *out_rgb, bool snaps) {
    rg_aa_res &r = s->aa;
    for (uint32_t b = 0; b < p.bands; ++b) {
        const int i = (int)(b & 1u);
        hipStream_t rs = r.rs[i];
        rg_launch_desc d;
        d.width = p.k * p.width;
        d.height = p.k * p.host_rows;
        d.tiling = rg_tiling{p.k * p.band_rows, p.bands, b};  // exactly sample rows [b k band_rows, (b + 1) k band_rows)
        d.rgba = static_cast<uint8_t *>(r.slot_rgba[i]);
        d.rgb = static_cast<float *>(r.slot_rgb[i]);
        d.stream = rs;
        d.snap = snaps ? r.h_snap + 4 * (size_t)b : nullptr;
        const rg_status st = rg_launch_tiles(s, d);
        if (st != RG_OK) return st;
        const size_t off = (size_t)b * p.band_rows * p.width;  // the last band is partial: only rows below host_rows
        if (!ok(rg_launch_resolve(d.rgb, p.width, rg_band_rows(p, b), p.k, out_rgba + off * 4,
                                  out_rgb ? out_rgb + off * 3 : nullptr, rs)) ||
            !ok(hipEventRecord(r.ev_done[b], rs)))
            return RG_ERR_DEVICE;
    }
    return RG_OK;
}

// Rays summed over the bands; a device error names the OUTPUT pixel that contains the
// lowest-index failing sample of the k W x k H frame.  kernel_ms: first render .. last resolve.
rg_status aa_stats(const rg_scene *s, const aa_plan &p, rg_stats *stats) {
    rg_aa_res &r = s->aa;
    rg_stats total;
    const rg_status err = rg_finish_stats(r.h_snap, (int)p.bands, r.ev_t0, r.ev_t1, &total);
    if (err != RG_OK) {
        const uint32_t e = (uint32_t)total.error_pixel, kw = p.k * p.width;
        total.error_pixel = (int32_t)((e / kw / p.k) * p.width + (e % kw) / p.k);
    }
    if (stats) *stats = total;
    return err;
}

rg_status render_aa_host(const rg_scene *s, const aa_plan &p, uint8_t *rgba_out, float *rgb_out, rg_stats *stats) {
    rg_aa_res &r = s->aa;
    rg_status st = ensure_aa_res(s, p);
    if (st != RG_OK) return st;
    const bool want_rgb = rgb_out != nullptr;
    if ((st = rg_bands_ensure_frame(r, (size_t)p.host_rows * p.width, want_rgb)) != RG_OK) return st;
    uint8_t *d_rgba = static_cast<uint8_t *>(r.d_rgba);
    float *d_rgb = want_rgb ? static_cast<float *>(r.d_rgb) : nullptr;
    if (!rg_bands_fork(r)) return RG_ERR_DEVICE;
    if ((st = enqueue_bands(s, p, d_rgba, d_rgb, true)) != RG_OK) return rg_bands_drain(r, st);
    if (!rg_bands_join(r)) return rg_bands_drain(r, RG_ERR_DEVICE);
    if ((st = rg_bands_deliver(r, p, d_rgba, d_rgb, rgba_out, rgb_out)) != RG_OK) return st;
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
    rg_status st = ensure_aa_res(s, p);
    if (st != RG_OK) return st;
    rg_aa_res &r = s->aa;
    hipStream_t caller = static_cast<hipStream_t>(stream);
    // the scene's two streams fork from the caller's stream and join it again
    if (!ok(hipEventRecord(r.ev_fork, caller)) || !ok(hipStreamWaitEvent(r.rs[0], r.ev_fork, 0)) ||
        !ok(hipStreamWaitEvent(r.rs[1], r.ev_fork, 0)) || !ok(hipEventRecord(r.ev_t0, r.rs[0])))
        return RG_ERR_DEVICE;
    st = enqueue_bands(s, p, rgba_dev, rgb_dev, snaps);
    const bool joined = rg_bands_join(r) && ok(hipStreamWaitEvent(caller, r.ev_t1, 0));
    if (st != RG_OK || !joined) return rg_bands_drain(r, st != RG_OK ? st : RG_ERR_DEVICE);
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
