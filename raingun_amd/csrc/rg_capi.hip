// rg_capi.hip — the host-visible part of the C ABI declared in
// include/raingun.h: frames delivered into host memory (banded renders
// overlapped with their device-to-host copies, one launch writing page-locked
// memory, the split of the two), streaming bands, host buffer registration,
// the batch closest-hit query and the debug setters.  The scene is in
// rg_scene.hip, the tiled launch every path here goes through in
// rg_launch.hip, the streams, events and buffers of a banded frame, its
// delivery to the caller and the stats tail of every path here in rg_bands.hip,
// the band arithmetic in rg_band_plan.h, the pageable-frame copy pool in
// rg_copy_pool.cpp, the single-process multi-GPU entry (rg_render_multi) in
// rg_multi.hip (the dealing of tiles it and rg_frames.hip share in rg_tile_deal.h, their
// pack and re-interleave kernels in rg_gather.hip, the RCCL loader in rg_rccl.hip), the
// supersampled frames (rg_render_image_aa) in rg_aa.hip, the AOV pass in rg_aov.hip, the
// ambient occlusion pass in rg_ao.hip and the ambient term in rg_ambient.hip (their shared
// launch path, rg_pass_enqueue, in rg_launch.hip).  The blocking entries here and there keep
// their device scratch in an rg_scratch (rg_internal.h), which frees it when they return.
// Once a path here has enqueued work that stores into the caller's buffer,
// every error exit drains its streams first (rg_bands_drain).  No exception or
// abort crosses the ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/raingun.h"
#include "../../include/raingun_debug.h"
#include "rg_device.h"
#include "rg_exact.h"
#include "rg_internal.h"
#include "rg_launchers.h"

#pragma clang fp contract(off)

#ifndef RG_LANE_MIN_DEPTH
#define RG_LANE_MIN_DEPTH 1
#endif

void rg_image_res_release(rg_image_res &r) {
    rg_bands_release(r);  // first: it waits for the streams
    if (r.h_frame) (void)hipHostFree(r.h_frame);
    if (r.h_flags) (void)hipHostFree(r.h_flags);
    if (r.h_cancel) (void)hipHostFree(r.h_cancel);
    r = rg_image_res{};
}

void *rg_host_device_ptr(void *p, size_t bytes) {
    if (!p || bytes == 0) return nullptr;
    auto dev = [](void *q) -> char * {
        hipPointerAttribute_t at;
        std::memset(&at, 0, sizeof at);
        if (hipPointerGetAttributes(&at, q) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        return at.type == hipMemoryTypeHost ? static_cast<char *>(at.devicePointer) : nullptr;
    };
    char *d0 = dev(p), *d1 = dev(static_cast<char *>(p) + bytes - 1);
    // one mapping: the last byte's device address continues the first's
    return (d0 && d1 && d1 == d0 + (bytes - 1)) ? d0 : nullptr;
}

bool rg_host_is_pinned(const void *p, size_t bytes) {
    if (!p || bytes == 0) return false;
    auto one = [](const void *q) {
        hipPointerAttribute_t at;
        std::memset(&at, 0, sizeof at);
        if (hipPointerGetAttributes(&at, q) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        return at.type == hipMemoryTypeHost;
    };
    return one(p) && one(static_cast<const char *>(p) + bytes - 1);
}

uint32_t rg_host_tile_wlog(const rg_scene *s) {
    return (uint32_t)(s->host_tile_forced || rg_scene_heavy(s) ? s->host_tile_wlog : RG_HOST_TILE_WLOG_LIGHT);
}

extern "C" {

int32_t rg_abi_version(void) { return RG_ABI_VERSION; }

const char *rg_status_string(int32_t st) {
    switch (st) {
    case RG_OK: return "ok";
    case RG_ERR_INVALID_ARGUMENT: return "invalid argument";
    case RG_ERR_PORTRAIT: return "width must be >= height (ray.rs:42)";
    case RG_ERR_AABB_NORMAL: return "could not determine normal of point (bodies.rs:324)";
    case RG_ERR_NAN_DISTANCE: return "NaN intersection distance compared (scene.rs:38)";
    case RG_ERR_TRANSMISSION: return "transmission ray is None while kr < 1 (rendering.rs:106)";
    case RG_ERR_TEXTURE: return "texture index out of range or empty texture";
    case RG_ERR_DEVICE: return "HIP runtime error";
    case RG_ERR_OUT_OF_MEMORY: return "out of device memory";
    case RG_ERR_CANCELLED: return "cancelled by the tile callback";
    case RG_ERR_COLLECTIVE: return "RCCL unavailable or failed (rg_render_multi)";
    case RG_ERR_PENDING: return "a frame batch waits for its gather: rg_frames_flush on every rank first";
    default: return "unknown status";
    }
}

int32_t rg_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

}  // extern "C"

// ---------------------------------------------------------------- host-visible frames
// The drop-in for rendering::render_image (rendering.rs:24-38) returns the
// frame in HOST memory: rendered in row bands (rg_band_plan.h) and delivered
// band by band (rg_bands.hip), or written over PCIe by the kernel itself.
// Device framebuffer, staging, streams and events belong to the scene and are
// reused across calls.
namespace {

// The scene's band resource set (rg_bands.h), for `bands` bands.
rg_status ensure_image_res(const rg_scene *s, uint32_t bands) {
    // The host frame's two render streams run concurrently (split frames: the device part on
    // rs[0], the one-launch part on rs[1]), so they must not share a hardware queue.  HIP hands a
    // plain new stream one of the process's shared queues, and where it lands depends on the
    // streams made before it: two of three test1 instances ran the split frame at 1.06 ms instead
    // of 0.76-0.80 (the parts serialised) after the bench reused its render streams
    // (profiles/r06/s32, s36).  A stream with a CU mask (every CU) gets a hardware queue of its
    // own: rs[1] is made so.  rs[0] stays a plain stream -- the heavy scenes' one-launch frame runs
    // there, and on a CU-masked queue it measured 2.32 instead of 2.03 ms in two of three runs (s37).
    return rg_bands_ensure(s->img, s->device, bands, RG_IMAGE_STREAM_CUMASK != 0);
}

// Wait until tiles [t0, t1) of the launch carry `seq` (the kernel publishes a
// tile after a system-scope release of its pixels).  Polls the launch's done
// event now and then, so a failed launch returns instead of spinning.
rg_status wait_tiles(const uint32_t *flags, size_t t0, size_t t1, uint32_t seq, hipEvent_t done) {
    unsigned spins = 0;
    for (size_t i = t0; i < t1; ++i) {
        while (__atomic_load_n(&flags[i], __ATOMIC_ACQUIRE) != seq) {
            if ((++spins & 1023u) == 0u) {
                const hipError_t e = hipEventQuery(done);
                if (e == hipSuccess) {  // the kernel is done: the flag must be there now
                    if (__atomic_load_n(&flags[i], __ATOMIC_ACQUIRE) != seq) return RG_ERR_DEVICE;
                } else if (e != hipErrorNotReady) {
                    (void)hipGetLastError();
                    return RG_ERR_DEVICE;
                }
            }
            __builtin_ia32_pause();
        }
    }
    return RG_OK;
}

// What every launch of the host-visible paths sets; each path adds its own fields.
rg_launch_desc frame_launch(uint32_t W, uint32_t H, const rg_tiling &t, void *rgba, hipStream_t stream,
                            unsigned long long *snap) {
    rg_launch_desc d;
    d.width = W;
    d.height = H;
    d.tiling = t;
    d.rgba = static_cast<uint8_t *>(rgba);
    d.stream = stream;
    d.snap = snap;
    return d;
}

// The tile grid of a one-launch host frame of `rows` rows in 2^wlog-wide tiles, as the kernel
// counts it (rg_device.h rg_tiles_x / rg_tiles_y): tile height, tiles across, tile rows, tiles.
struct host_grid {
    uint32_t TH;
    size_t tiles_x, tile_rows, ntiles;
};
host_grid host_tile_grid(uint32_t W, uint32_t rows, uint32_t wlog) {
    const uint32_t TH = 64u >> wlog;
    const size_t tiles_x = ((size_t)W + (1u << wlog) - 1u) >> wlog, tile_rows = (rows + TH - 1u) / TH;
    return {TH, tiles_x, tile_rows, tiles_x * tile_rows};
}

// Host-visible frame in ONE launch, no device framebuffer and no copy engine:
// the kernel's pixel stores go straight over PCIe into page-locked host memory
// (8x8-tile-shaped 4-B stores reach 52.7 GB/s of the 55.8 GB/s a DMA copy
// does: profiles/r02/host_visible/d2h_probe.jsonl), so the transfer overlaps the whole
// render.  A pinned caller buffer is written directly.  A pageable one
// (a Rust Vec, a numpy array) is fed from a pinned frame the kernel writes:
// the kernel publishes each finished 8x8 tile (RgKernelArgs::tile_flags) and
// the host copies every band of rows, on RG_COPY_HELPERS + 1 threads, as
// soon as its tiles are in, while the kernel renders the rest.
rg_status render_host_direct(const rg_scene *s, uint32_t W, uint32_t H, const rg_tiling *t, uint32_t rows,
                             uint8_t *rgba_out, rg_stats *stats) {
    rg_image_res &r = s->img;
    const size_t row4 = (size_t)W * 4, bytes = (size_t)rows * row4;
    hipStream_t rs = r.rs[0];
    void *dst = rg_host_device_ptr(rgba_out, std::max<size_t>(bytes, 1));
    const bool pageable = dst == nullptr;
    const uint32_t wl = rg_host_tile_wlog(s);
    const auto [TH, tiles_x, tile_rows, ntiles] = host_tile_grid(W, rows, wl);
    rg_status st = RG_OK;
    uint32_t seq = 0;
    if (pageable) {
        if ((st = rg_grow(RG_MEM_PINNED_ZEROED, r.h_frame, r.h_frame_cap, bytes + 4)) != RG_OK) return st;
        if ((st = rg_grow(RG_MEM_PINNED_ZEROED, r.h_flags, r.h_flags_cap, (ntiles + 1) * 4)) != RG_OK) return st;
        dst = rg_host_device_ptr(r.h_frame, std::max<size_t>(bytes, 1));
        if (!dst) return RG_ERR_DEVICE;
        if (++r.seq == 0) r.seq = 1;
        seq = r.seq;
    }
    uint32_t *flags_dev = nullptr;
    if (pageable && !(flags_dev = static_cast<uint32_t *>(rg_host_device_ptr(r.h_flags, ntiles * 4 + 4))))
        return RG_ERR_DEVICE;
    if (!ok(hipEventRecord(r.ev_t0, rs))) return RG_ERR_DEVICE;
    rg_launch_desc d = frame_launch(W, H, *t, dst, rs, r.h_snap);
    d.tile_flags = flags_dev;
    d.frame_seq = seq;
    d.tile_wlog = wl;
    d.host_frame = true;
    // from here on the kernel may be storing into the caller's buffer: error exits drain
    st = rg_launch_tiles(s, d);
    if (st != RG_OK) return rg_bands_drain(r, st);
    if (!ok(hipEventRecord(r.ev_t1, rs))) return rg_bands_drain(r, RG_ERR_DEVICE);
    if (pageable) {
        rg_copy_pool &pool = rg_bands_pool(r);
        rg_copy_pool::Active active(pool);
        // bands of whole tile rows, ~RG_IMAGE_BAND_PX / 4 pixels each (the queue hands out tiles in raster order)
        const size_t band_tr = std::max<size_t>(1, (RG_IMAGE_BAND_PX / 4) / ((size_t)W * TH));
        for (size_t tr0 = 0; tr0 < tile_rows && st == RG_OK; tr0 += band_tr) {
            const size_t tr1 = std::min(tile_rows, tr0 + band_tr);
            if ((st = wait_tiles(r.h_flags, tr0 * tiles_x, tr1 * tiles_x, seq, r.ev_t1)) != RG_OK) break;
            const size_t y0 = tr0 * TH, y1 = std::min<size_t>(rows, tr1 * TH);
            pool.copy(rgba_out + y0 * row4, static_cast<uint8_t *>(r.h_frame) + y0 * row4, (y1 - y0) * row4);
        }
    }
    if (!ok(hipStreamSynchronize(rs))) return rg_bands_drain(r, RG_ERR_DEVICE);
    if (st != RG_OK) return st;
    return rg_finish_stats(r.h_snap, 1, r.ev_t0, r.ev_t1, stats);
}

// Host-visible frame into a page-locked buffer, split in two concurrent parts
// that share the PCIe link: the top rows render into device memory (a plain
// device-resident launch) and go to the caller's buffer as one DMA copy, while
// the rest is ONE launch writing its pixels over PCIe itself
// (render_host_direct's kernel).  The one-launch kernel alone reaches ~38 GB/s
// of the ~55 GB/s a copy does; the copy of the first part runs beside it.
// The automatic choice for light-path scenes into page-locked buffers (test1
// 4K 0.90 -> 0.80 ms, test3 0.835 -> 0.80: profiles/r05/s31, s32); heavy
// scenes keep the one launch (north star 2.13 -> 2.23-2.70 ms split).
#ifndef RG_HOST_SPLIT_PCT
#define RG_HOST_SPLIT_PCT 35
#endif
rg_status render_host_split(const rg_scene *s, uint32_t W, uint32_t H, const rg_tiling *t, uint32_t rows,
                            uint8_t *rgba_out, rg_stats *stats) {
    (void)t;  // a whole-frame tiling (stride 1): output row = image row
    rg_image_res &r = s->img;
    const size_t row4 = (size_t)W * 4;
    void *dst = rg_host_device_ptr(rgba_out, (size_t)rows * row4);
    if (!dst) return RG_ERR_INVALID_ARGUMENT;  // pinned buffers only (the caller checked)
    // the frame re-cut into 8-row tiles (the caller's tiling is a whole-frame one: output row = image row)
    const rg_tiling t8 = {8u, 1u, 0u};
    const uint32_t TR = 8u, nt = (H + 7u) / 8u;
    const int pct = s->host_split_pct > 0 ? s->host_split_pct : RG_HOST_SPLIT_PCT;
    const uint32_t ja = std::min(nt - 1u, std::max(1u, (uint32_t)(((unsigned long long)nt * (unsigned)pct + 50u) / 100u)));
    const size_t a_bytes = (size_t)ja * TR * row4;  // rows [0, ja TR): below H (ja < nt)
    if (rows > H) std::memset(rgba_out + (size_t)H * row4, 0, (size_t)(rows - H) * row4);  // the tiling's padding
    rg_status st = rg_bands_ensure_frame(r, (size_t)ja * TR * W, false);
    if (st != RG_OK) return st;
    if (!rg_bands_fork(r)) return RG_ERR_DEVICE;
    // Once either part is enqueued, every exit first drains both render streams and the copy
    // stream: part B's kernel and part A's DMA store into the caller's buffer.
    // part A (device memory): tiles [0, ja) of the frame
    auto launch_a = [&]() -> rg_status {
        if (s->split_fail_a > 0) {  // rg_debug_fail_split_a: this launch reports failure without running
            --s->split_fail_a;
            return RG_ERR_DEVICE;
        }
        rg_launch_desc d = frame_launch(W, H, t8, r.d_rgba, r.rs[0], r.h_snap);
        d.tile_count = ja;
        const rg_status e = rg_launch_tiles(s, d);
        if (e != RG_OK) return e;
        return ok(hipEventRecord(r.ev_done[0], r.rs[0])) ? RG_OK : RG_ERR_DEVICE;
    };
    // part B (one launch writing host memory): tiles from ja on, to image rows >= ja * 8
    auto launch_b = [&]() -> rg_status {
        rg_launch_desc d = frame_launch(W, H, t8, dst, r.rs[1], r.h_snap + 4);
        d.tile_wlog = rg_host_tile_wlog(s);
        d.host_frame = true;
        d.image_rows = true;
        d.tile_first = ja;
        return rg_launch_tiles(s, d);
    };
    // part B's persistent host-frame launch first, part A's beside it: B's PCIe writes start at once
    // (test1 4K pinned 0.854 -> 0.80 ms at 35 %; 30 % 0.83, 40 % 0.91: profiles/r05/s32)
    if ((st = launch_b()) != RG_OK || (st = launch_a()) != RG_OK) return rg_bands_drain(r, st);
    if (!ok(hipStreamWaitEvent(r.cs, r.ev_done[0], 0)) ||
        !ok(hipMemcpyAsync(rgba_out, r.d_rgba, a_bytes, hipMemcpyDeviceToHost, r.cs)) ||
        !ok(hipEventRecord(r.ev_copy[0], r.cs)) || !ok(hipStreamWaitEvent(r.rs[1], r.ev_copy[0], 0)) ||
        !ok(hipEventRecord(r.ev_t1, r.rs[1])))
        return rg_bands_drain(r, RG_ERR_DEVICE);
    const bool synced1 = ok(hipStreamSynchronize(r.rs[1]));
    const bool synced0 = ok(hipStreamSynchronize(r.rs[0]));
    if (!synced1 || !synced0) return rg_bands_drain(r, RG_ERR_DEVICE);
    return rg_finish_stats(r.h_snap, 2, r.ev_t0, r.ev_t1, stats);  // part A holds the lower pixel indices: its error first
}

}  // namespace

rg_status rg_render_host(const rg_scene *s, uint32_t W, uint32_t H, const rg_tiling *t, uint8_t *rgba_out,
                         float *rgb_out, rg_stats *stats) {
    if (!s || !rgba_out || W == 0 || H == 0 || !rg_tiling_valid(t)) return RG_ERR_INVALID_ARGUMENT;
    if (W < H) return RG_ERR_PORTRAIT;
    const uint32_t rows = rg_tiling_rows(H, t);
    if ((unsigned long long)rows * W >= (1ull << 32) || (unsigned long long)H * W >= (1ull << 32))
        return RG_ERR_INVALID_ARGUMENT;
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    // A whole-frame tiling (stride 1) is re-cut into K bands of BR rows (tiling {BR, K, b}
    // renders exactly rows [b BR, (b+1) BR)); a sharded tiling is rendered in one launch.
    const bool banded = t->tile_stride == 1;
    const rg_band_plan p = banded ? rg_image_band_plan(s->image_bands, W, H, RG_IMAGE_BAND_PX) : rg_one_band(W, rows);
    rg_status st = ensure_image_res(s, std::max(p.bands, 2u));  // the split frame has two parts
    if (st != RG_OK) return st;
    rg_image_res &r = s->img;
    // Path choice (4K frames): into page-locked buffers one launch writing host
    // memory wins -- heavy scenes (synth1024: 2.99 vs 3.63 ms banded,
    // profiles/r02/host_visible/hv_sweep.jsonl) and, since the light path stores
    // its tiles through an LDS ring in contiguous 4-KB runs of 64x1 tiles, light
    // scenes too (test1 0.86 vs 0.93 ms, test3 0.82 vs 0.84:
    // profiles/r03/late/hv_ring_group.txt); into pageable memory the per-tile
    // publication costs more than the copies it overlaps (test1 2.5 vs 1.15
    // ms) -- banded there.
    if (!rgb_out) {
        const bool pinned = rg_host_device_ptr(rgba_out, std::max<size_t>((size_t)rows * W * 4, 1)) != nullptr;
        const bool split = s->image_bands == -2 || (s->image_bands == 0 && !rg_scene_heavy(s));
        if (split && pinned && t->tile_stride == 1 && H >= 16)
            return render_host_split(s, W, H, t, rows, rgba_out, stats);
        bool direct = s->image_bands < 0;
        if (s->image_bands == 0) direct = pinned;
        if (direct) return render_host_direct(s, W, H, t, rows, rgba_out, stats);
    }

    const bool want_rgb = rgb_out != nullptr;
    const size_t row4 = (size_t)W * 4, row12 = (size_t)W * 12;
    if ((st = rg_bands_ensure_frame(r, (size_t)p.bands * p.band_rows * W, want_rgb)) != RG_OK) return st;
    uint8_t *d_rgba = static_cast<uint8_t *>(r.d_rgba);
    float *d_rgb = want_rgb ? static_cast<float *>(r.d_rgb) : nullptr;
    if (!rg_bands_fork(r)) return RG_ERR_DEVICE;
    for (uint32_t b = 0; b < p.bands; ++b) {
        hipStream_t rs = r.rs[b & 1];
        const rg_tiling bt = banded ? rg_tiling{p.band_rows, p.bands, b} : *t;
        const size_t off = (size_t)b * p.band_rows * W;
        rg_launch_desc d = frame_launch(W, H, bt, d_rgba + off * 4, rs, r.h_snap + 4 * b);
        if (want_rgb) d.rgb = d_rgb + off * 3;
        if ((st = rg_launch_tiles(s, d)) != RG_OK) return rg_bands_drain(r, st);
        if (!ok(hipEventRecord(r.ev_done[b], rs))) return rg_bands_drain(r, RG_ERR_DEVICE);
    }
    if (!rg_bands_join(r)) return rg_bands_drain(r, RG_ERR_DEVICE);
    if ((st = rg_bands_deliver(r, p, d_rgba, d_rgb, rgba_out, rgb_out)) != RG_OK) return st;
    if (banded && rows > H) {  // padding rows of a whole-frame tiling whose tile_rows does not divide H
        std::memset(rgba_out + (size_t)H * row4, 0, (size_t)(rows - H) * row4);
        if (want_rgb) std::memset(rgb_out + (size_t)H * W * 3, 0, (size_t)(rows - H) * row12);
    }
    return rg_finish_stats(r.h_snap, (int)p.bands, r.ev_t0, r.ev_t1, stats);
}

extern "C" {

rg_status rg_render_tiles(const rg_scene *s, uint32_t width, uint32_t height, const rg_tiling *tiling,
                          uint8_t *rgba_out, float *rgb_out, rg_stats *stats) {
    return rg_render_host(s, width, height, tiling, rgba_out, rgb_out, stats);
}

rg_status rg_render_image(const rg_scene *s, uint32_t width, uint32_t height, uint8_t *rgba_out, rg_stats *stats) {
    rg_tiling whole = {height ? height : 1, 1, 0};
    return rg_render_host(s, width, height, &whole, rgba_out, nullptr, stats);
}

rg_status rg_host_register(void *ptr, size_t bytes) {
    if (!ptr || bytes == 0) return RG_ERR_INVALID_ARGUMENT;
    // portable: every device's DMA engine may write it (rg_render_multi's per-device copies)
    if (!ok(hipHostRegister(ptr, bytes, hipHostRegisterPortable))) {
        (void)hipGetLastError();
        return RG_ERR_DEVICE;
    }
    return RG_OK;
}

rg_status rg_host_unregister(void *ptr) {
    if (!ptr) return RG_ERR_INVALID_ARGUMENT;
    if (!ok(hipHostUnregister(ptr))) {
        (void)hipGetLastError();
        return RG_ERR_DEVICE;
    }
    return RG_OK;
}

// Tile-completion streaming (render_image_stream, rendering.rs:40-69): ONE
// launch of the whole frame writes its pixels over PCIe into a pinned,
// coherent host frame and publishes every finished 8x8 tile
// (RgKernelArgs::tile_flags); the host hands band after band of `tile_rows`
// rows to the callback, in row order, as soon as the band's tiles are in,
// while the kernel renders the rest.  A callback returning nonzero cancels:
// the kernel takes no further tiles (RgKernelArgs::cancel; the reference's
// `.all` short-circuits likewise) and the call returns RG_ERR_CANCELLED once
// the tiles in flight are done.
rg_status rg_render_stream(const rg_scene *s, uint32_t width, uint32_t height, uint32_t tile_rows,
                           rg_tile_callback on_tile, void *user, rg_stats *stats) {
    if (!s || !on_tile || width == 0 || height == 0 || tile_rows == 0) return RG_ERR_INVALID_ARGUMENT;
    if (width < height) return RG_ERR_PORTRAIT;
    if ((unsigned long long)height * width >= (1ull << 32)) return RG_ERR_INVALID_ARGUMENT;
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    rg_status st = ensure_image_res(s, 1);
    if (st != RG_OK) return st;
    rg_image_res &r = s->img;
    const size_t row4 = (size_t)width * 4, bytes = (size_t)height * row4;
    const uint32_t wl = (uint32_t)s->host_tile_wlog;
    const auto [TH, tiles_x, grid_rows, ntiles] = host_tile_grid(width, height, wl);
    (void)grid_rows;
    size_t cancel_cap = r.h_cancel ? 64 : 0;
    if ((st = rg_grow(RG_MEM_PINNED_ZEROED, r.h_frame, r.h_frame_cap, bytes + 4)) != RG_OK ||
        (st = rg_grow(RG_MEM_PINNED_ZEROED, r.h_flags, r.h_flags_cap, (ntiles + 1) * 4)) != RG_OK ||
        (st = rg_grow(RG_MEM_PINNED_ZEROED, r.h_cancel, cancel_cap, 64)) != RG_OK)
        return st;
    void *frame_dev = rg_host_device_ptr(r.h_frame, bytes);
    uint32_t *flags_dev = static_cast<uint32_t *>(rg_host_device_ptr(r.h_flags, ntiles * 4 + 4));
    const uint32_t *cancel_dev = static_cast<const uint32_t *>(rg_host_device_ptr(r.h_cancel, 4));
    if (!frame_dev || !flags_dev || !cancel_dev) return RG_ERR_DEVICE;
    __atomic_store_n(r.h_cancel, 0u, __ATOMIC_RELEASE);
    if (++r.seq == 0) r.seq = 1;
    const uint32_t seq = r.seq;
    hipStream_t rs = r.rs[0];
    const rg_tiling whole = {height, 1, 0};
    if (!ok(hipEventRecord(r.ev_t0, rs))) return RG_ERR_DEVICE;
    rg_launch_desc d = frame_launch(width, height, whole, frame_dev, rs, r.h_snap);
    d.tile_flags = flags_dev;
    d.frame_seq = seq;
    d.cancel = cancel_dev;
    d.tile_wlog = wl;
    d.host_frame = true;
    // from here on error exits drain: the callback's bands are read from a frame the kernel writes
    st = rg_launch_tiles(s, d);
    if (st != RG_OK) return rg_bands_drain(r, st);
    if (!ok(hipEventRecord(r.ev_t1, rs))) return rg_bands_drain(r, RG_ERR_DEVICE);
    const uint8_t *frame = static_cast<const uint8_t *>(r.h_frame);
    for (uint32_t y0 = 0; y0 < height; y0 += tile_rows) {
        const uint32_t n = std::min(tile_rows, height - y0);
        if ((st = wait_tiles(r.h_flags, (size_t)(y0 / TH) * tiles_x, ((size_t)(y0 + n) + TH - 1u) / TH * tiles_x, seq,
                             r.ev_t1)) != RG_OK)
            break;
        if (on_tile(y0, n, width, frame + (size_t)y0 * row4, user) != 0) {
            __atomic_store_n(r.h_cancel, 1u, __ATOMIC_RELEASE);
            st = RG_ERR_CANCELLED;
            break;
        }
    }
    if (!ok(hipStreamSynchronize(rs))) return rg_bands_drain(r, RG_ERR_DEVICE);
    const rg_status err = rg_finish_stats(r.h_snap, 1, r.ev_t0, r.ev_t1, stats);
    if (st == RG_OK && err != RG_OK) return err;
    return st;
}

rg_status rg_debug_set_path(rg_scene *s, int32_t path) {
    if (!s || path < RG_PATH_AUTO || path > RG_PATH_HEAVY) return RG_ERR_INVALID_ARGUMENT;
    s->path = path;
    return RG_OK;
}

rg_status rg_debug_set_bvh(rg_scene *s, int32_t enable) {
    if (!s || (enable != 0 && enable != 1)) return RG_ERR_INVALID_ARGUMENT;
    s->bvh_enabled = enable != 0;
    return RG_OK;
}

rg_status rg_debug_set_lightbuf(rg_scene *s, int32_t enable) {
    if (!s || (enable != 0 && enable != 1)) return RG_ERR_INVALID_ARGUMENT;
    s->lbuf_enabled = enable != 0;
    return RG_OK;
}

int32_t rg_debug_lightbuf_count(const rg_scene *s) {
    // buffers IN USE: none while the BVH or the buffers are switched off (rg_debug_set_lightbuf(0))
    if (!s || !s->host || !s->bvh_enabled || !s->lbuf_enabled || s->n_nodes == 0) return 0;
    int32_t n = 0;
    for (int32_t i = 0; i < s->n_lbuf; ++i) n += s->host->lbuf[(size_t)i].kind != RG_LB_NONE;
    return n;
}

rg_status rg_debug_bvh_info(const rg_scene *s, rg_bvh_info *info) {
    if (!s || !info) return RG_ERR_INVALID_ARGUMENT;
    *info = s->bvh_info;
    info->enabled = s->bvh_enabled && s->n_nodes > 0;
    return RG_OK;
}

rg_status rg_debug_set_lane_depth(rg_scene *s, int32_t min_depth) {
    if (!s) return RG_ERR_INVALID_ARGUMENT;
    s->lane_min_depth = min_depth < 0 ? RG_LANE_MIN_DEPTH : min_depth;
    return RG_OK;
}

rg_status rg_debug_set_tile_order(rg_scene *s, int32_t mode) {
    if (!s || mode < -1 || mode > 1) return RG_ERR_INVALID_ARGUMENT;
    s->tile_order = mode;
    return RG_OK;
}

rg_status rg_debug_set_image_bands(rg_scene *s, int32_t bands) {
    if (!s || bands < -2 || bands > RG_IMAGE_MAX_BANDS) return RG_ERR_INVALID_ARGUMENT;
    s->image_bands = bands;
    return RG_OK;
}

rg_status rg_debug_set_host_split(rg_scene *s, int32_t pct) {
    if (!s || pct < 0 || pct > 99) return RG_ERR_INVALID_ARGUMENT;
    s->host_split_pct = pct;
    return RG_OK;
}

rg_status rg_debug_set_host_ring(rg_scene *s, int32_t flush_small, int32_t group_small, int32_t flush_big,
                                  int32_t group_big, int32_t multi_light_one) {
    if (!s || flush_small < -1 || flush_small > 16 || group_small < -1 || flush_big < -1 || flush_big > 16 ||
        group_big < -1 || multi_light_one < -1 || multi_light_one > 1)
        return RG_ERR_INVALID_ARGUMENT;
    if (flush_small >= 0) s->ring_flush_small = flush_small;
    if (group_small >= 0) s->ring_group_small = group_small;
    if (flush_big >= 0) s->ring_flush_big = flush_big;
    if (group_big >= 0) s->ring_group_big = group_big;
    if (multi_light_one >= 0) s->multi_light_one = multi_light_one != 0;
    return RG_OK;
}

rg_status rg_debug_fail_split_a(rg_scene *s, int32_t count) {
    if (!s || count < 0) return RG_ERR_INVALID_ARGUMENT;
    s->split_fail_a = count;
    return RG_OK;
}

rg_status rg_debug_set_host_tile_shape(rg_scene *s, int32_t tile_wlog) {
    if (!s || !(tile_wlog == 0 || (tile_wlog >= 3 && tile_wlog <= 6))) return RG_ERR_INVALID_ARGUMENT;
    s->host_tile_wlog = tile_wlog == 0 ? RG_HOST_TILE_WLOG : tile_wlog;
    s->host_tile_forced = tile_wlog != 0;
    return RG_OK;
}

rg_status rg_debug_counters(const rg_scene *s, uint64_t out[16]) {
    if (!s || !out) return RG_ERR_INVALID_ARGUMENT;
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    if (!ok(hipStreamSynchronize(s->last->stream)) ||
        !ok(hipMemcpy(out, s->last->last_counters, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost)))
        return RG_ERR_DEVICE;
    return RG_OK;
}

rg_status rg_debug_last_plain(const rg_scene *s, int32_t *plain) {
    if (!s || !plain || !s->last) return RG_ERR_INVALID_ARGUMENT;
    *plain = s->last->last_plain;
    return RG_OK;
}

rg_status rg_debug_set_shadow_volume(rg_scene *s, int32_t on) {
    if (!s || (on != 0 && on != 1)) return RG_ERR_INVALID_ARGUMENT;
    s->shvol_enabled = on != 0;
    return RG_OK;
}

rg_status rg_debug_shadow_volume_info(const rg_scene *s, rg_shadow_volume_info *info) {
    if (!s || !info) return RG_ERR_INVALID_ARGUMENT;
    *info = s->shvol_info;
    info->enabled = s->shvol_info.built && s->shvol_enabled;
    return RG_OK;
}

rg_status rg_debug_last_shadow_volume(const rg_scene *s, int32_t *used) {
    if (!s || !used || !s->last) return RG_ERR_INVALID_ARGUMENT;
    *used = s->last->last_shvol;
    return RG_OK;
}

rg_status rg_debug_set_first_hit_tiles(rg_scene *s, int32_t on) {
    if (!s || (on != 0 && on != 1)) return RG_ERR_INVALID_ARGUMENT;
    s->first_hit_enabled = on != 0;
    return RG_OK;
}

rg_status rg_debug_last_first_hit_tiles(const rg_scene *s, uint64_t *tiles) {
    if (!s || !tiles || !s->last) return RG_ERR_INVALID_ARGUMENT;
    return rg_debug_counter_words(s, RG_FIRST_HIT_WORD, 1, tiles);
}

rg_status rg_debug_set_exact_div(rg_scene *s, int32_t enable) {
    if (!s || (enable != 0 && enable != 1)) return RG_ERR_INVALID_ARGUMENT;
    s->exact_div = enable != 0;
    return RG_OK;
}

rg_status rg_debug_camera_check(const rg_scene *s, uint32_t width, uint32_t height, double fov, uint64_t *mismatches,
                                int32_t *admitted) {
    if (!s || !mismatches || width == 0 || height == 0 || (unsigned long long)width * height >= (1ull << 32))
        return RG_ERR_INVALID_ARGUMENT;
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    RgKernelArgs a = rg_make_args(s);
    a.width = width;
    a.height = height;
    a.width_d = (double)width;
    a.height_d = (double)height;
    a.aspect = a.width_d / a.height_d;
    a.fov_adjustment = rg_fov_adjustment(fov);
    a.inv_w = 1.0 / a.width_d;
    a.inv_h = 1.0 / a.height_d;
    if (admitted)
        *admitted = rg_recip_div_ok(width) && rg_recip_div_ok(height) && rg_camera_unscaled_ok(a.fov_adjustment, a.aspect);
    rg_scratch mem;
    unsigned long long *d_bad = mem.dev<unsigned long long>(sizeof(unsigned long long)), bad = 0;
    if (mem.status() != RG_OK) return mem.status();
    rg_status st = RG_OK;
    if (!ok(hipMemset(d_bad, 0, sizeof bad)) || !ok(rg_launch_camera_check(&a, d_bad, nullptr)) ||
        !ok(hipMemcpy(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost)))
        st = RG_ERR_DEVICE;
    *mismatches = bad;
    return st;
}

rg_status rg_debug_unscaled_check(const rg_scene *s, int32_t op, const double *a, const double *b, uint32_t n,
                                  uint64_t *mismatches) {
    if (!s || !a || !mismatches || n == 0 || n > (1u << 24) || op < 0 || op > 3 || (op == 2 && !b))
        return RG_ERR_INVALID_ARGUMENT;
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    const size_t bytes = (size_t)n * sizeof(double);
    unsigned long long bad = 0;
    *mismatches = 0;
    rg_scratch mem;
    double *d_a = mem.dev<double>(bytes), *d_b = op == 2 ? mem.dev<double>(bytes) : nullptr;
    double *d_out = mem.dev<double>(2 * bytes);
    unsigned long long *d_bad = mem.dev<unsigned long long>(sizeof bad);
    if (mem.status() != RG_OK) return mem.status();
    if (!ok(hipMemcpy(d_a, a, bytes, hipMemcpyHostToDevice)) ||
        (op == 2 && !ok(hipMemcpy(d_b, b, bytes, hipMemcpyHostToDevice))) || !ok(hipMemset(d_out, 0, 2 * bytes)) ||
        !ok(hipMemset(d_bad, 0, sizeof bad)) || !ok(rg_launch_unscaled_check(op, d_a, d_b, n, d_out, d_bad, nullptr)) ||
        !ok(hipMemcpy(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost)))
        return RG_ERR_DEVICE;
    *mismatches = bad;
    return RG_OK;
}

rg_status rg_debug_counter_words(const rg_scene *s, int32_t first, int32_t n, uint64_t *out) {
    if (!s || !out || first < 0 || n < 0 || first + n > RG_COUNTER_WORDS) return RG_ERR_INVALID_ARGUMENT;
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    if (!ok(hipStreamSynchronize(s->last->stream)) ||
        !ok(hipMemcpy(out, s->last->last_counters + first, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost)))
        return RG_ERR_DEVICE;
    return RG_OK;
}

rg_status rg_trace(const rg_scene *s, const double *rays, uint32_t n, double *dist, int32_t *body) {
    if (!s || (n && (!rays || !dist || !body))) return RG_ERR_INVALID_ARGUMENT;
    if (n == 0) return RG_OK;
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    rg_scratch mem;
    double *d_rays = mem.dev<double>((size_t)n * 48), *d_dist = mem.dev<double>((size_t)n * 8);
    int32_t *d_body = mem.dev<int32_t>((size_t)n * 4);
    if (mem.status() != RG_OK) return mem.status();
    rg_launch_ctx *cx = rg_ctx_for(s, nullptr);
    if (!cx) return RG_ERR_OUT_OF_MEMORY;
    s->last = cx;
    RgKernelArgs a = rg_make_args(s);
    // the trace kernel counts into the set the context's next render launch will
    // use, and re-zeroes it after the read-back (that launch expects it zeroed)
    unsigned long long *cs = cx->counters + (size_t)cx->cur * RG_COUNTER_WORDS, c[4] = {0, 0, 0, 0};
    a.counters = cs;
    if (!ok(hipMemcpy(d_rays, rays, (size_t)n * 48, hipMemcpyHostToDevice)) || !ok(hipMemset(cs, 0, sizeof c)) ||
        !ok(rg_launch_trace(&a, d_rays, n, d_dist, d_body, nullptr)) ||
        !ok(hipMemcpy(dist, d_dist, (size_t)n * 8, hipMemcpyDeviceToHost)) ||
        !ok(hipMemcpy(body, d_body, (size_t)n * 4, hipMemcpyDeviceToHost)) ||
        !ok(hipMemcpy(c, cs, sizeof c, hipMemcpyDeviceToHost)) ||
        !ok(hipMemset(cs, 0, RG_COUNTER_WORDS * sizeof(unsigned long long))))
        return RG_ERR_DEVICE;
    return rg_snap_status(c, nullptr);  // RG_OK without an error word
}

}  // extern "C"
