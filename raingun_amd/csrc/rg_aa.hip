// rg_aa.hip — supersampled anti-aliasing: samples x samples rays per pixel on the
// regular sub-pixel grid, box-filtered (rg_render_image_aa, rg_render_aa_async,
// rg_resolve_box, rg_debug_set_aa_band_rows), and its adaptive form, which traces the
// samples only of pixels on edges of the 1-sample frame (rg_render_image_aa_adaptive,
// rg_render_aa_adaptive, rg_edge_mask: "adaptive" below).
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

#include <cstring>

#include "../../include/raingun.h"
#include "../../include/raingun_debug.h"
#include "rg_device.h"
#include "rg_internal.h"
#include "rg_launchers.h"
#include "rg_area.h"
#include "rg_lens.h"
#include "rg_sample_tiles.h"

#pragma clang fp contract(off)

void rg_aa_res_release(rg_aa_res &r) {
    rg_bands_release(r);  // first: it waits for the streams
    if (r.base_stream) { (void)hipStreamSynchronize(r.base_stream); (void)hipStreamDestroy(r.base_stream); }
    if (r.ev_fork) (void)hipEventDestroy(r.ev_fork);
    if (r.ev_list) (void)hipEventDestroy(r.ev_list);
    for (hipEvent_t e : r.ev_mark) (void)hipEventDestroy(e);
    if (r.d_mask) (void)hipFree(r.d_mask);
    if (r.d_list) (void)hipFree(r.d_list);
    if (r.d_counts) (void)hipFree(r.d_counts);
    if (r.h_counts) (void)hipHostFree(r.h_counts);
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

aa_plan aa_make_plan(const rg_scene *s, uint32_t W, uint32_t H, uint32_t k, size_t slot_bytes = RG_AA_SLOT_BYTES) {
    return {rg_aa_band_plan(s->aa_band_rows, W, H, k, slot_bytes, RG_AA_MIN_BAND_ROWS), k};
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
    // a frame through the scene's lens: the tables, once per scene (a blocking copy: they are complete
    // before the first launch that reads them is enqueued, and nothing writes them again)
    // (a frame with area lights reads the turns of the same tables)
    if ((rg_lens_active(s->lens.aperture, p.k) || rg_area_active(s->area_any, p.k)) && !r.d_lens) {
        double table[RG_LENS_TABLE_DOUBLES];
        rg_lens_make_tables(table);
        if ((st = rg_table_once(s, r.d_lens, table, sizeof table)) != RG_OK) return st;
    }
    // a replica's area table, which rg_scene_set_light_radii of the scene it copies did not write
    if (rg_area_active(s->area_any, p.k) && (s->area_stale || !s->d_area)) {
        if ((st = rg_area_upload(const_cast<rg_scene *>(s))) != RG_OK) return st;
    }
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
        d.lens_k = p.k;  // the samples of a pixel leave the scene's lens, if it has one (k >= 2)
        d.lens_tab = r.d_lens;
        d.area_tab = s->d_area;  // ... and see its lights with their radii, if any has one
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

// ---------------------------------------------------------------- adaptive
// rg_render_image_aa_adaptive / rg_render_aa_adaptive: the 1-sample frame (one launch into the
// W x H result), its edge mask and, per band of the plan, the list of the 8x8 sample tiles
// that hold a sample of a flagged pixel (rg_edge.hip), all on base_stream; the host waits for
// the flagged count and the per-band list lengths; then the bands with a non-empty list
// alternate between the two render streams as above: a sparse launch of the list into the
// band's slot (only the samples of flagged pixels are traced) and the adaptive resolve
// (rg_resolve.hip), which overwrites the flagged pixels of the result.  Counter snapshots:
// h_snap[4 b ..] band b (zero when skipped), h_snap[4 bands ..] the 1-sample frame.

// d_counts / h_counts: per band its listed tiles, then (on a 128-B line) the mask kernel's sharded flagged counters.
size_t adaptive_shard_base(uint32_t bands) { return ((size_t)bands + RG_EDGE_SHARD_WORDS - 1) / RG_EDGE_SHARD_WORDS * RG_EDGE_SHARD_WORDS; }
size_t adaptive_count_words(uint32_t bands) { return adaptive_shard_base(bands) + (size_t)RG_EDGE_SHARDS * RG_EDGE_SHARD_WORDS; }

// The adaptive paths' own resources, beside ensure_aa_res's; own_mask: the mask goes to d_mask.
rg_status ensure_adaptive_res(const rg_scene *s, const aa_plan &p, bool own_mask) {
    rg_aa_res &r = s->aa;
    rg_status st = rg_bands_ensure(r, s->device, p.bands + 1, false);  // + the base frame's snapshot
    if (st != RG_OK) return st;
    if (!r.base_stream && !ok(hipStreamCreateWithFlags(&r.base_stream, hipStreamNonBlocking))) return RG_ERR_DEVICE;
    if (!r.ev_list && !ok(hipEventCreateWithFlags(&r.ev_list, hipEventDisableTiming))) return RG_ERR_DEVICE;
    if (own_mask && (st = rg_grow(RG_MEM_DEVICE, r.d_mask, r.d_mask_cap, (size_t)p.width * p.host_rows + 16)) != RG_OK)
        return st;
    const size_t stride = rg_sample_tile_count(p.width, p.band_rows, p.k);
    if ((st = rg_grow(RG_MEM_DEVICE, r.d_list, r.d_list_cap, (size_t)p.bands * stride * 4 + 16)) != RG_OK) return st;
    const size_t words = adaptive_count_words(p.bands);
    if ((st = rg_grow(RG_MEM_DEVICE, r.d_counts, r.d_counts_cap, words * 4)) != RG_OK) return st;
    return rg_grow(RG_MEM_PINNED, r.h_counts, r.h_counts_cap, words * 4);
}

// Every stream of the adaptive paths idle (rg_bands_drain + base_stream).
rg_status adaptive_drain(rg_aa_res &r, rg_status status) {
    if (r.base_stream) (void)hipStreamSynchronize(r.base_stream);
    return rg_bands_drain(r, status);
}

// The passes.  base_stream is ordered behind whatever the frame must follow; d_rgba / d_rgb
// (nullable) / d_mask: the W x H result in device memory.  Blocks between the passes; returns
// with the bands enqueued and ev_done[b] recorded for every band.
rg_status adaptive_passes(const rg_scene *s, const aa_plan &p, uint32_t threshold, uint8_t *d_rgba, float *d_rgb,
                          uint8_t *d_mask) {
    rg_aa_res &r = s->aa;
    hipStream_t bs = r.base_stream;
    const uint32_t W = p.width, H = p.host_rows, k = p.k, nb = p.bands;
    const uint32_t stride = rg_sample_tile_count(W, p.band_rows, k);
    std::memset(r.h_snap, 0, ((size_t)nb + 1) * 4 * sizeof(unsigned long long));  // a skipped band counts nothing
    // the probe's timing events (rg_debug_set_aa_adaptive_timing): 4 on base_stream, then 3 per band
    r.n_marks = 0;
    auto mark = [&r](hipStream_t st) -> bool {
        if (!r.timing) return true;
        if (r.n_marks == r.ev_mark.size()) {
            hipEvent_t e = nullptr;
            if (!ok(hipEventCreate(&e))) return false;
            r.ev_mark.push_back(e);
        }
        return ok(hipEventRecord(r.ev_mark[r.n_marks++], st));
    };
    if (!mark(bs)) return RG_ERR_DEVICE;
    rg_launch_desc base;
    base.width = W;
    base.height = H;
    base.tiling = rg_tiling{H, 1, 0};
    base.rgba = d_rgba;
    base.rgb = d_rgb;
    base.stream = bs;
    base.snap = r.h_snap + 4 * (size_t)nb;
    rg_status st = rg_launch_tiles(s, base);
    if (st != RG_OK) return st;
    const size_t shards = adaptive_shard_base(nb), words = adaptive_count_words(nb);
    if (!ok(hipMemsetAsync(r.d_counts, 0, words * 4, bs)) || !mark(bs) ||
        !ok(rg_launch_edge_mask(d_rgba, W, H, threshold, d_mask, r.d_counts + shards, bs)) || !mark(bs) ||
        (k >= 2 && !ok(rg_launch_tile_list(d_mask, W, H, k, p.band_rows, nb, r.d_list, stride, r.d_counts, bs))) ||
        !mark(bs) || !ok(hipMemcpyAsync(r.h_counts, r.d_counts, words * 4, hipMemcpyDeviceToHost, bs)) ||
        !ok(hipEventRecord(r.ev_list, bs)) || !ok(hipEventSynchronize(r.ev_list)))
        return RG_ERR_DEVICE;
    r.flagged = 0;
    for (size_t i = 0; i < RG_EDGE_SHARDS; ++i) r.flagged += r.h_counts[shards + i * RG_EDGE_SHARD_WORDS];
    r.listed_tiles = r.bands_launched = 0;
    // the render streams' work is enqueued after the wait above: it follows the base frame, the mask and the lists
    for (uint32_t b = 0; b < nb; ++b) {
        const int i = (int)(b & 1u);
        hipStream_t rs = r.rs[i];
        const uint32_t listed = k >= 2 ? r.h_counts[b] : 0u;
        const size_t off = (size_t)b * p.band_rows * W;
        if (!mark(rs)) return RG_ERR_DEVICE;
        if (listed > 0) {
            r.listed_tiles += listed;
            r.bands_launched += 1;
            rg_launch_desc d;
            d.width = k * W;
            d.height = k * H;
            d.tiling = rg_tiling{k * p.band_rows, nb, b};
            d.rgba = static_cast<uint8_t *>(r.slot_rgba[i]);
            d.rgb = static_cast<float *>(r.slot_rgb[i]);
            d.stream = rs;
            d.snap = r.h_snap + 4 * (size_t)b;
            d.tile_list = r.d_list + (size_t)b * stride;
            d.tile_limit = listed;
            d.px_mask = d_mask;
            d.px_k = k;
            d.px_w = W;
            if ((st = rg_launch_tiles(s, d)) != RG_OK) return st;
        }
        if (!mark(rs)) return RG_ERR_DEVICE;
        // a band without flagged pixels still has its f32 RGB clamped (the k = 1 resolve)
        if ((listed > 0 || d_rgb) &&
            !ok(rg_launch_resolve_adaptive(listed > 0 ? static_cast<const float *>(r.slot_rgb[i]) : nullptr, d_mask + off, W,
                                           rg_band_rows(p, b), k, d_rgba + off * 4, d_rgb ? d_rgb + off * 3 : nullptr, rs)))
            return RG_ERR_DEVICE;
        if (!mark(rs) || !ok(hipEventRecord(r.ev_done[b], rs))) return RG_ERR_DEVICE;
    }
    return RG_OK;
}

// The probe's times, once every stream is idle.
void adaptive_pass_times(rg_aa_res &r) {
    for (float &m : r.pass_ms) m = 0.0f;
    auto span = [&r](size_t a, size_t b) {
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, r.ev_mark[a], r.ev_mark[b]);
        return ms;
    };
    if (r.n_marks < 4) return;
    for (size_t m = 0; m < 3; ++m) r.pass_ms[m] = span(m, m + 1);
    for (size_t m = 4; m + 2 < r.n_marks; m += 3) {
        r.pass_ms[3] += span(m, m + 1);
        r.pass_ms[4] += span(m + 1, m + 2);
    }
}

// Rays of the base frame plus the bands'.  A device error: the lower of the base pass's failing
// pixel and the output pixel that contains the lowest-index failing traced sample (aa_stats'
// mapping), with that pixel's status; on a tie the base pass's, which is folded first.
rg_status adaptive_stats(const rg_scene *s, const aa_plan &p, rg_stats *stats) {
    rg_aa_res &r = s->aa;
    rg_stats bands, base;
    adaptive_pass_times(r);
    const rg_status err_bands = aa_stats(s, p, &bands);
    const rg_status err_base = rg_snap_status(r.h_snap + 4 * (size_t)p.bands, &base);
    rg_stats total{};
    total.kernel_ms = bands.kernel_ms;
    total.error_pixel = -1;
    rg_status err = RG_OK;
    rg_stats_add(total, err, base, err_base);
    rg_stats_add(total, err, bands, err_bands);
    if (stats) *stats = total;
    return err;
}

rg_status adaptive_check(const void *scene, uint32_t W, uint32_t H, uint32_t k, uint32_t threshold, const void *rgba) {
    const rg_status v = aa_validate(scene, W, H, k, rgba);
    if (v != RG_OK) return v;
    // no adaptive form through a lens: the edge mask comes from a pinhole frame and says nothing about defocus
    if (static_cast<const rg_scene *>(scene)->lens.aperture > 0.0) return RG_ERR_INVALID_ARGUMENT;
    // nor with area lights: the mask comes from a hard-shadow frame and says nothing about penumbrae
    if (static_cast<const rg_scene *>(scene)->area_any) return RG_ERR_INVALID_ARGUMENT;
    return threshold > 256 ? RG_ERR_INVALID_ARGUMENT : RG_OK;
}

}  // namespace

extern "C" {

rg_status rg_render_image_aa_adaptive(const rg_scene *s, uint32_t width, uint32_t height, uint32_t samples,
                                      uint32_t threshold, uint8_t *rgba_out, float *rgb_out, uint8_t *mask_out,
                                      rg_stats *stats) {
    const rg_status v = adaptive_check(s, width, height, samples, threshold, rgba_out);
    if (v != RG_OK) return v;
    if (threshold == 0) {  // every pixel is flagged: the full form, no base pass
        if (mask_out) std::memset(mask_out, 1, (size_t)width * height);
        return rg_render_image_aa(s, width, height, samples, rgba_out, rgb_out, stats);
    }
    if (samples == 1 && !rgb_out && !mask_out) return rg_render_image(s, width, height, rgba_out, stats);
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    const aa_plan p = aa_make_plan(s, width, height, samples, RG_AA_ADAPTIVE_SLOT_BYTES);
    rg_aa_res &r = s->aa;
    rg_status st = ensure_aa_res(s, p);
    if (st != RG_OK || (st = ensure_adaptive_res(s, p, true)) != RG_OK) return st;
    const bool want_rgb = rgb_out != nullptr;
    if ((st = rg_bands_ensure_frame(r, (size_t)height * width, want_rgb)) != RG_OK) return st;
    uint8_t *d_rgba = static_cast<uint8_t *>(r.d_rgba);
    float *d_rgb = want_rgb ? static_cast<float *>(r.d_rgb) : nullptr;
    if (!ok(hipEventRecord(r.ev_t0, r.base_stream))) return RG_ERR_DEVICE;
    if ((st = adaptive_passes(s, p, threshold, d_rgba, d_rgb, r.d_mask)) != RG_OK) return adaptive_drain(r, st);
    if (!rg_bands_join(r)) return adaptive_drain(r, RG_ERR_DEVICE);
    // the mask is final since the wait between the passes
    if (mask_out && !ok(hipMemcpy(mask_out, r.d_mask, (size_t)width * height, hipMemcpyDeviceToHost)))
        return adaptive_drain(r, RG_ERR_DEVICE);
    if ((st = rg_bands_deliver(r, p, d_rgba, d_rgb, rgba_out, rgb_out)) != RG_OK) return st;
    return adaptive_stats(s, p, stats);
}

rg_status rg_render_aa_adaptive(const rg_scene *s, uint32_t width, uint32_t height, uint32_t samples, uint32_t threshold,
                                uint8_t *rgba_dev, float *rgb_dev, uint8_t *mask_dev, void *stream, rg_stats *stats) {
    const rg_status v = adaptive_check(s, width, height, samples, threshold, rgba_dev);
    if (v != RG_OK) return v;
    hipStream_t caller = static_cast<hipStream_t>(stream);
    rg_stats local;
    if (threshold == 0 || (samples == 1 && !rgb_dev && !mask_dev)) {  // the full form / the 1-sample frame, blocking
        if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
        if (mask_dev && !ok(hipMemsetAsync(mask_dev, 1, (size_t)width * height, caller))) return RG_ERR_DEVICE;
        return rg_render_aa_async(s, width, height, samples, rgba_dev, rgb_dev, stream, stats ? stats : &local);
    }
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    const aa_plan p = aa_make_plan(s, width, height, samples, RG_AA_ADAPTIVE_SLOT_BYTES);
    rg_aa_res &r = s->aa;
    rg_status st = ensure_aa_res(s, p);
    if (st != RG_OK || (st = ensure_adaptive_res(s, p, mask_dev == nullptr)) != RG_OK) return st;
    // the scene's streams fork from the caller's stream and join it again
    if (!ok(hipEventRecord(r.ev_fork, caller)) || !ok(hipStreamWaitEvent(r.base_stream, r.ev_fork, 0)) ||
        !ok(hipEventRecord(r.ev_t0, r.base_stream)))
        return RG_ERR_DEVICE;
    st = adaptive_passes(s, p, threshold, rgba_dev, rgb_dev, mask_dev ? mask_dev : r.d_mask);
    const bool joined = rg_bands_join(r) && ok(hipStreamWaitEvent(caller, r.ev_t1, 0));
    if (st != RG_OK || !joined) return adaptive_drain(r, st != RG_OK ? st : RG_ERR_DEVICE);
    if (!ok(hipStreamSynchronize(caller))) return RG_ERR_DEVICE;
    return adaptive_stats(s, p, stats);
}

rg_status rg_edge_mask(int32_t device, const uint8_t *rgba_in, uint32_t width, uint32_t height, uint32_t threshold,
                       uint8_t *mask_out, uint32_t *flagged) {
    if (device < 0 || !rgba_in || !mask_out || width == 0 || height == 0 || threshold > 256 ||
        (unsigned long long)width * height >= (1ull << 32))
        return RG_ERR_INVALID_ARGUMENT;
    if (!ok(hipSetDevice(device))) return RG_ERR_DEVICE;
    const size_t px = (size_t)width * height;
    const size_t n_bytes = (size_t)RG_EDGE_SHARDS * RG_EDGE_SHARD_WORDS * 4;
    std::vector<uint32_t> shard(n_bytes / 4);
    rg_scratch mem;
    uint8_t *d_in = mem.dev<uint8_t>(px * 4), *d_mask = mem.dev<uint8_t>(px + 16);
    uint32_t *d_n = mem.dev<uint32_t>(n_bytes);
    if (mem.status() != RG_OK) return mem.status();
    if (!ok(hipMemcpy(d_in, rgba_in, px * 4, hipMemcpyHostToDevice)) || !ok(hipMemset(d_n, 0, n_bytes)) ||
        !ok(rg_launch_edge_mask(d_in, width, height, threshold, d_mask, d_n, nullptr)) ||
        !ok(hipMemcpy(mask_out, d_mask, px, hipMemcpyDeviceToHost)) ||
        !ok(hipMemcpy(shard.data(), d_n, n_bytes, hipMemcpyDeviceToHost)))
        return RG_ERR_DEVICE;
    uint32_t n = 0;
    for (size_t i = 0; i < RG_EDGE_SHARDS; ++i) n += shard[i * RG_EDGE_SHARD_WORDS];
    if (flagged) *flagged = n;
    return RG_OK;
}

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
    rg_scratch mem;
    float *d_in = mem.dev<float>(in_bytes);
    uint8_t *d_rgba = mem.dev<uint8_t>(px * 4);
    float *d_rgb = rgb_out ? mem.dev<float>(px * 12) : nullptr;
    if (mem.status() != RG_OK) return mem.status();
    if (!ok(hipMemcpy(d_in, rgb_in, in_bytes, hipMemcpyHostToDevice)) ||
        !ok(rg_launch_resolve(d_in, width, height, samples, d_rgba, d_rgb, nullptr)) ||
        !ok(hipMemcpy(rgba_out, d_rgba, px * 4, hipMemcpyDeviceToHost)) ||
        (rgb_out && !ok(hipMemcpy(rgb_out, d_rgb, px * 12, hipMemcpyDeviceToHost))))
        return RG_ERR_DEVICE;
    return RG_OK;
}

rg_status rg_debug_set_aa_adaptive_timing(rg_scene *s, int32_t enable) {
    if (!s) return RG_ERR_INVALID_ARGUMENT;
    s->aa.timing = enable != 0;
    return RG_OK;
}

rg_status rg_debug_aa_adaptive_info(const rg_scene *s, float ms[5], uint32_t *flagged, uint32_t *listed_tiles,
                                    uint32_t *bands_launched) {
    if (!s) return RG_ERR_INVALID_ARGUMENT;
    if (ms)
        for (int m = 0; m < 5; ++m) ms[m] = s->aa.pass_ms[m];
    if (flagged) *flagged = s->aa.flagged;
    if (listed_tiles) *listed_tiles = s->aa.listed_tiles;
    if (bands_launched) *bands_launched = s->aa.bands_launched;
    return RG_OK;
}

rg_status rg_debug_set_aa_band_rows(rg_scene *s, int32_t rows) {
    if (!s || rows < 0) return RG_ERR_INVALID_ARGUMENT;
    s->aa_band_rows = rows;
    return RG_OK;
}

}  // extern "C"
