// rg_launch.hip — the tiled launch behind every render path: the per-stream
// launch contexts (ray counters, error words, tile-order scratch, deep frame
// buffer, primary-ray table), the frame arguments every launch shares
// (rg_frame_args), the launch path of the pixel passes (rg_pass_check,
// rg_pass_enqueue, rg_pass_grid), rg_launch_tiles (validate, fill the kernel
// arguments, size the deep frame buffer, refresh the primary-ray table, order
// the tiles, launch and snapshot the counters), the decoding of counter
// snapshots, and the device-resident entries of the C ABI
// (rg_render_tiles_async / _pipelined, rg_stream_status).  No exception or
// abort crosses the ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/raingun.h"
#include "../../include/raingun_debug.h"
#include "rg_device.h"
#include "rg_exact.h"
#include "rg_internal.h"
#include "rg_launchers.h"
#include "rg_area.h"
#include "rg_lens.h"

#pragma clang fp contract(off)

namespace {

int frames_needed(uint32_t max_depth) { return max_depth > 1 ? (int)max_depth - 1 : 1; }

// decode the complemented error key of counters[3] / a sticky word
rg_status decode_error(unsigned long long word, int32_t *pixel) {
    if (word == 0) return RG_OK;
    const unsigned long long key = ~word;
    if (pixel) *pixel = (int32_t)(key >> 8);
    return (rg_status)(-(int32_t)(key & 0xff));
}

// The steps of rg_launch_tiles, in the order it takes them.

// 1. The first failing check decides the status.  out_rows: the rows this launch renders.
rg_status validate(const rg_scene *s, const rg_launch_desc &d, uint32_t *out_rows) {
    if (d.tile_wlog < 3 || d.tile_wlog > 6) return RG_ERR_INVALID_ARGUMENT;
    if (d.image_rows && (!d.host_frame || d.rgb)) return RG_ERR_INVALID_ARGUMENT;
    if (d.px_mask && (!d.tile_list || d.tile_limit == 0 || d.px_k == 0 || d.host_frame || d.tile_wlog != 3 ||
                      d.tile_flags || d.cancel))
        return RG_ERR_INVALID_ARGUMENT;
    if (!s || !d.rgba || d.width == 0 || d.height == 0 || !rg_tiling_valid(&d.tiling)) return RG_ERR_INVALID_ARGUMENT;
    if (d.lens_k && (d.px_mask || d.host_frame || d.tile_wlog != 3 || d.lens_k > RG_LENS_MAX_SAMPLES ||
                     d.width % d.lens_k != 0 || (rg_lens_active(s->lens.aperture, d.lens_k) && !d.lens_tab)))
        return RG_ERR_INVALID_ARGUMENT;
    if (rg_area_active(s->area_any, d.lens_k) && (!d.area_tab || !d.lens_tab)) return RG_ERR_INVALID_ARGUMENT;
    if (rg_lens_active(s->lens.aperture, d.lens_k) && s->has_camera) {
        // the lens disk's axes are the camera's right and up, normalized: a zero (or overflowing) one spans no disk
        double lr[3], lu[3];
        rg_lens_axis(s->camera.right, s->lens.aperture, lr);
        rg_lens_axis(s->camera.up, s->lens.aperture, lu);
        if (!rg_camera_finite3(lr) || !rg_camera_finite3(lu)) return RG_ERR_INVALID_ARGUMENT;
    }
    if (d.tile_group < 1 ||
        d.tiling.tile_offset + d.tile_group > d.tiling.tile_stride + (d.tile_group == 1 ? 1u : 0u))
        return RG_ERR_INVALID_ARGUMENT;
    if (d.width < d.height) return RG_ERR_PORTRAIT;  // ray.rs:42
    const uint32_t sel_rows = rg_tiling_rows_grouped(d.height, &d.tiling, d.tile_group);  // every selected tile
    const uint32_t sel_tiles = sel_rows / d.tiling.tile_rows;
    if (d.tile_first > sel_tiles) return RG_ERR_INVALID_ARGUMENT;
    *out_rows = std::min(sel_tiles - d.tile_first, d.tile_count) * d.tiling.tile_rows;
    if ((unsigned long long)*out_rows * d.width >= (1ull << 32) ||
        (unsigned long long)d.height * d.width >= (1ull << 32))
        return RG_ERR_INVALID_ARGUMENT;  // the reference's u32 pixel index (rendering.rs:27)
    return RG_OK;
}

// 2. The frame's arguments (rg_frame_args) plus this launch's band, quotients, lens, area lights, outputs and ring.
RgKernelArgs fill_args(const rg_scene *s, const rg_launch_desc &d, rg_launch_ctx *cx, uint32_t out_rows) {
    RgKernelArgs a = rg_frame_args(s, cx, d.width, d.height, d.tiling, d.tile_group, out_rows);
    a.tile_base = d.tile_first;
    // the PLAIN kernels' camera quotients (rg_exact.h): every column and row of a frame size swept
    // once per launch context (n divisions for n pixels a side), then remembered
    if (cx->rdiv_w != d.width || cx->rdiv_h != d.height) {
        cx->rdiv_ok = rg_recip_div_ok(d.width) && rg_recip_div_ok(d.height);
        cx->rdiv_w = d.width;
        cx->rdiv_h = d.height;
    }
    a.inv_w = 1.0 / a.width_d;
    a.inv_h = 1.0 / a.height_d;
    a.plain_veto = (cx->rdiv_ok && s->exact_div) ? 0u : 1u;
    if (a.camera) a.plain_veto |= 4u;  // the PLAIN kernels' camera ray is the reference's view
    if (rg_lens_active(s->lens.aperture, d.lens_k)) {  // by value, as the camera
        if (!a.camera) {  // the reference's view as a camera: the lens family is the camera family's
            a.camera = 1u;
            a.cam_right[0] = a.cam_up[1] = 1.0;
            a.cam_forward[2] = -1.0;
            a.plain_veto |= 4u;
        }
        a.lens = 1u;
        a.lens_k = d.lens_k;
        a.lens_focus = s->lens.focus;
        rg_lens_axis(a.cam_right, s->lens.aperture, a.lens_r);
        rg_lens_axis(a.cam_up, s->lens.aperture, a.lens_u);
        a.lens_tab = d.lens_tab;
    }
    if (rg_area_active(s->area_any, d.lens_k)) {  // by reference: the scene's device table (rg_scene_set_light_radii)
        if (!a.camera) {  // the reference's view as a camera: the area family is the camera family's
            a.camera = 1u;
            a.cam_right[0] = a.cam_up[1] = 1.0;
            a.cam_forward[2] = -1.0;
            a.plain_veto |= 4u;
        }
        a.lens_k = d.lens_k;
        a.lens_tab = d.lens_tab;  // the turns
        a.area_tab = d.area_tab;
    }
    a.rgba = reinterpret_cast<uint32_t *>(d.rgba);
    a.rgb = d.rgb;
    a.tile_flags = d.tile_flags;
    a.frame_seq = d.frame_seq;
    a.cancel = d.cancel;
    a.tile_wlog = d.tile_wlog;
    a.defer_px = d.host_frame ? 1u : 0u;
    a.image_rows = d.image_rows ? 1u : 0u;
    a.pipelined = d.pipelined ? 1u : 0u;
    if (d.px_mask) {  // a sparse launch: the list is the queue
        a.px_mask = d.px_mask;
        a.px_k = d.px_k;
        a.px_w = d.px_w;
        a.tile_perm = d.tile_list;
        a.tile_limit = d.tile_limit;
    }
    if (d.host_frame) {  // the light path's LDS tile ring (rg_device.h RG_RING_*)
        const bool big = rg_tile_count(a) >= RG_RING_BIG_TILES;
        a.ring_flush = (uint32_t)std::max(0, big ? s->ring_flush_big : s->ring_flush_small);
        a.ring_group = (uint32_t)std::max(0, big ? s->ring_group_big : s->ring_group_small);
    }
    // the PLAIN kernels' tile start (RgKernelArgs::tiles_x_m ..): divisions by launch constants
    const RgMagicU32 mx = rg_magic_u32(rg_tiles_x(a)), mr = rg_magic_u32(a.tile_rows);
    a.tiles_x_m = mx.m;
    a.tiles_x_sh = mx.sh;
    a.tile_rows_m = mr.m;
    a.tile_rows_sh = mr.sh;
    a.tile_rows_shift = 32u;
    for (uint32_t k = 0; k < 32u; ++k)
        if (a.tile_rows == 1u << k) a.tile_rows_shift = k;
    a.rows_identity = (a.tile_stride == 1u && a.tile_offset == 0u && a.tile_base == 0u && a.tile_group <= 1u &&
                       a.out_tile_mul <= 1u)
                          ? 1u
                          : 0u;
    return a;
}

// 3. Kernels whose frames live in a global buffer (depth `disp`): the buffer, sized for this
// launch's (persistent) grid.
rg_status size_deep_frames(rg_launch_ctx *cx, RgKernelArgs &a, int frames, int disp) {
    if (!rg_launch_global_frames(&a, disp) || a.out_rows == 0) return RG_OK;
    size_t threads = 0;
    if (!ok(rg_render_grid_threads(&a, disp, &threads)) || threads == 0 || threads > 0xFFFFFFFFull)
        return RG_ERR_DEVICE;
    const size_t per_thread = (size_t)frames * RG_FRAME_BYTES;
    if (threads * per_thread > ((size_t)1 << 30)) {
        // very deep recursion (scene.rs:16 is a u32): a persistent grid that fits half the free
        // device memory (at most 16 GiB of frames) -- fewer waves, every depth still renders
        size_t free_b = 0, total_b = 0;
        if (!ok(hipMemGetInfo(&free_b, &total_b))) return RG_ERR_DEVICE;
        const size_t budget = std::min<size_t>(free_b / 2, (size_t)16 << 30);
        if (threads * per_thread > budget) {
            a.max_grid_threads = (uint32_t)std::min<size_t>(budget / per_thread, 0xFFFFFFFFu);
            if (!ok(rg_render_grid_threads(&a, disp, &threads)) || threads == 0) return RG_ERR_DEVICE;
            if (threads * per_thread > budget) return RG_ERR_OUT_OF_MEMORY;  // not even one block fits
        }
    }
    const rg_status st = rg_grow(RG_MEM_DEVICE, cx->deep, cx->deep_bytes, threads * per_thread);
    if (st != RG_OK) return st;
    a.deep_stack = cx->deep;
    a.deep_stride = (uint32_t)threads;
    return RG_OK;
}

// 4. Primary-ray sensor coordinates per column / row (ray.rs:46-51), the
// kernel's expressions evaluated here once per frame size (same IEEE
// operations in the same order, no contraction: identical doubles).
rg_status refresh_prim_table(rg_launch_ctx *cx, RgKernelArgs &a, hipStream_t st) {
    const uint32_t width = a.width, height = a.height;
    if (cx->prim_w != width || cx->prim_h != height || cx->prim_fov != a.fov_adjustment || !cx->prim) {
        const size_t n = (size_t)width + height;
        const rg_status g = rg_grow(RG_MEM_DEVICE, cx->prim, cx->prim_cap, n * sizeof(double));
        if (g != RG_OK) return g;
        std::vector<double> tab(n);
        for (uint32_t x = 0; x < width; ++x)
            tab[x] = ((((double)x + 0.5) / (double)width) * 2.0 - 1.0) * a.aspect * a.fov_adjustment;
        for (uint32_t y = 0; y < height; ++y)
            tab[(size_t)width + y] = (1.0 - (((double)y + 0.5) / (double)height) * 2.0) * a.fov_adjustment;
        // stream-ordered: earlier launches on this stream are done with the old table
        if (!ok(hipMemcpyAsync(cx->prim, tab.data(), n * sizeof(double), hipMemcpyHostToDevice, st)) ||
            !ok(hipStreamSynchronize(st)))
            return RG_ERR_DEVICE;
        cx->prim_w = width;
        cx->prim_h = height;
        cx->prim_fov = a.fov_adjustment;
    }
    a.prim_sx = cx->prim;
    a.prim_sy = cx->prim + width;
    return RG_OK;
}

// 5. Expensive tiles first on the heavy path (probe-ordered light tiles measured slower:
// DESIGN.md 4g); rg_debug_set_tile_order overrides.
rg_status order_tiles(const rg_scene *s, const rg_launch_desc &d, rg_launch_ctx *cx, RgKernelArgs &a) {
    if (!(s->tile_order == 1 || (s->tile_order < 0 && rg_heavy_path(a)))) return RG_OK;
    const size_t ntiles = (size_t)rg_tile_count(a);
    rg_launch_ctx::PermKey key{d.width, d.height, d.tiling.tile_rows, d.tiling.tile_stride,
                               d.tiling.tile_offset, d.tile_first, a.out_rows, d.tile_wlog, s->max_depth,
                               (uint32_t)s->n_lights, d.tile_group, a.fov_adjustment, s->mats};
    // the probe's rays are the launch's: an order made through one camera is not another's (nor the fixed view's)
    key.camera = a.camera != 0;
    for (int k = 0; key.camera && k < 3; ++k) {
        key.cam[k] = a.cam_eye[k];
        key.cam[3 + k] = a.cam_right[k];
        key.cam[6 + k] = a.cam_up[k];
        key.cam[9 + k] = a.cam_forward[k];
    }
    const bool cached = cx->perm_valid && cx->perm_key == key;
    // the pair under one capacity (in tiles); a failure here leaves the runtime's last error as it is
    if (!cached && rg_grow(RG_MEM_DEVICE, cx->tile_cap, ntiles,
                           {{cx->tile_cost, rg_tile_order_scratch_words((uint32_t)ntiles) * 4},
                            {cx->tile_perm, ntiles * 4}},
                           false) != RG_OK)
        return RG_ERR_OUT_OF_MEMORY;
    if (ntiles == 0) return RG_OK;
    // the order depends only on the frame geometry and the scene: made once per
    // launch context and key, so a steady stream of frames runs ONE kernel each
    if (!cached) {
        cx->perm_valid = false;
        if (!ok(rg_launch_tile_order(&a, cx->tile_cost, cx->tile_perm, d.stream))) return RG_ERR_DEVICE;
        cx->perm_valid = true;
        cx->perm_key = key;
    }
    a.tile_perm = cx->tile_perm;
    return RG_OK;
}

// 6. The render kernel, and the launch's statistics words: written into page-locked host
// memory by the kernel's last wave, or copied.
rg_status launch_and_snapshot(const rg_launch_desc &d, rg_launch_ctx *cx, RgKernelArgs &a, int disp) {
    hipStream_t st = d.stream;
    cx->last_counters = a.counters;
    unsigned long long *snap_dev =
        (d.snap && a.out_rows > 0)
            ? static_cast<unsigned long long *>(rg_host_device_ptr(d.snap, 4 * sizeof(*d.snap)))
            : nullptr;
    a.snap_out = snap_dev;
    if (a.out_rows > 0) {
        if (!ok(rg_launch_render(&a, disp, st, &cx->last_plain))) return RG_ERR_DEVICE;
        cx->last_shvol = cx->last_plain && a.shvol != nullptr;  // only the PLAIN kernels read it
        cx->cur = 1 - cx->cur;  // the kernel zeroes the other set for the next launch
    }
    if (d.timed && !ok(hipEventRecord(cx->ev1, st))) return RG_ERR_DEVICE;
    if (d.snap && !snap_dev &&
        !ok(hipMemcpyAsync(d.snap, a.counters, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st)))
        return RG_ERR_DEVICE;
    return RG_OK;
}

// The stats tail of a timed launch on cx's stream (ev0 .. ev1 recorded around it): wait for it, its time, the four
// counter words of its set.
rg_status stats_tail(rg_launch_ctx *cx, hipStream_t st, rg_stats *stats) {
    unsigned long long c[4];
    if (!ok(hipMemcpyAsync(c, cx->last_counters, sizeof c, hipMemcpyDeviceToHost, st)) || !ok(hipStreamSynchronize(st)))
        return RG_ERR_DEVICE;
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, cx->ev0, cx->ev1);
    stats->kernel_ms = ms;
    return rg_snap_status(c, stats);
}

// The ABI's device-resident renders (a null tiling stays invalid: rg_tiling{} selects nothing).
rg_launch_desc device_frame(uint32_t width, uint32_t height, const rg_tiling *tiling, uint8_t *rgba_dev,
                            float *rgb_dev, hipStream_t stream) {
    rg_launch_desc d;
    d.width = width;
    d.height = height;
    d.tiling = tiling ? *tiling : rg_tiling{};
    d.rgba = rgba_dev;
    d.rgb = rgb_dev;
    d.stream = stream;
    return d;
}

}  // namespace

void rg_ctx_destroy(rg_launch_ctx *c) {
    if (c->counters) (void)hipFree(c->counters);
    if (c->sticky) (void)hipFree(c->sticky);
    if (c->tile_cost) (void)hipFree(c->tile_cost);
    if (c->tile_perm) (void)hipFree(c->tile_perm);
    if (c->deep) (void)hipFree(c->deep);
    if (c->prim) (void)hipFree(c->prim);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    delete c;
}

rg_launch_ctx *rg_ctx_for(const rg_scene *s, hipStream_t stream) {
    for (rg_launch_ctx *c : s->ctxs)
        if (c->stream == stream) return c;
    rg_launch_ctx *c = new (std::nothrow) rg_launch_ctx();
    if (!c) return nullptr;
    c->stream = stream;
    void *p = nullptr, *q = nullptr;
    if (!ok(hipMalloc(&p, 2 * RG_COUNTER_WORDS * sizeof(unsigned long long)))) { delete c; return nullptr; }
    c->counters = static_cast<unsigned long long *>(p);
    c->last_counters = c->counters;
    // stream-ordered: hipMemset on the null stream does not order against a
    // non-blocking stream's first launch
    if (!ok(hipMemsetAsync(p, 0, 2 * RG_COUNTER_WORDS * sizeof(unsigned long long), stream))) {
        rg_ctx_destroy(c);
        return nullptr;
    }
    if (!ok(hipMalloc(&q, sizeof(unsigned long long))) || !ok(hipMemsetAsync(q, 0, sizeof(unsigned long long), stream))) {
        if (q) (void)hipFree(q);
        rg_ctx_destroy(c);
        return nullptr;
    }
    c->sticky = static_cast<unsigned long long *>(q);
    if (!ok(hipEventCreate(&c->ev0)) || !ok(hipEventCreate(&c->ev1))) {
        rg_ctx_destroy(c);
        return nullptr;
    }
    s->ctxs.push_back(c);
    return c;
}

rg_status rg_grow(rg_mem kind, size_t &cap, size_t want, std::initializer_list<rg_grow_buf> bufs, bool clear_error) {
    if (want <= cap) return RG_OK;
    for (const rg_grow_buf &b : bufs)
        if (*b.p) (void)(kind == RG_MEM_DEVICE ? hipFree(*b.p) : hipHostFree(*b.p));
    for (const rg_grow_buf &b : bufs) *b.p = nullptr;
    cap = 0;
    for (const rg_grow_buf &b : bufs) {
        void *q = nullptr;
        const hipError_t e = kind == RG_MEM_DEVICE   ? hipMalloc(&q, b.bytes)
                             : kind == RG_MEM_PINNED ? hipHostMalloc(&q, b.bytes, hipHostMallocDefault)
                                                     : hipHostMalloc(&q, b.bytes, hipHostMallocCoherent);
        if (!ok(e)) {
            if (clear_error) (void)hipGetLastError();
            return RG_ERR_OUT_OF_MEMORY;
        }
        if (kind == RG_MEM_PINNED_ZEROED) std::memset(q, 0, b.bytes);
        *b.p = q;
    }
    cap = want;
    return RG_OK;
}

RgKernelArgs rg_frame_args(const rg_scene *s, rg_launch_ctx *cx, uint32_t W, uint32_t H, const rg_tiling &t,
                           uint32_t tile_group, uint32_t out_rows) {
    RgKernelArgs a = rg_make_args(s);
    a.counters = cx->counters + (size_t)cx->cur * RG_COUNTER_WORDS;  // zero (see rg_launch_ctx::counters)
    a.counters_next = cx->counters + (size_t)(1 - cx->cur) * RG_COUNTER_WORDS;
    a.err_sticky = cx->sticky;
    a.width = W;
    a.height = H;
    a.tile_rows = t.tile_rows;
    a.tile_stride = t.tile_stride;
    a.tile_offset = t.tile_offset;
    a.tile_group = tile_group;
    a.out_rows = out_rows;
    a.width_d = (double)W;
    a.height_d = (double)H;
    a.aspect = a.width_d / a.height_d;
    if (s->has_camera) {  // by value: this launch keeps its camera whatever the scene is given next
        a.camera = 1u;
        for (int k = 0; k < 3; ++k) {
            a.cam_eye[k] = s->camera.eye[k];
            a.cam_right[k] = s->camera.right[k];
            a.cam_up[k] = s->camera.up[k];
            a.cam_forward[k] = s->camera.forward[k];
        }
    }
    return a;
}

rg_status rg_pass_check(const rg_scene *s, uint32_t W, uint32_t H, const rg_tiling *t, uint32_t *rows) {
    if (!s || W == 0 || H == 0 || !t || !rg_tiling_valid(t)) return RG_ERR_INVALID_ARGUMENT;
    if (W < H) return RG_ERR_PORTRAIT;  // ray.rs:42
    *rows = rg_tiling_rows(H, t);
    if ((unsigned long long)*rows * W >= (1ull << 32) || (unsigned long long)H * W >= (1ull << 32))
        return RG_ERR_INVALID_ARGUMENT;  // the reference's u32 pixel index (rendering.rs:27)
    return ok(hipSetDevice(s->device)) ? RG_OK : RG_ERR_DEVICE;
}

rg_status rg_pass_enqueue(const rg_scene *s, uint32_t W, uint32_t H, const rg_tiling &t, uint32_t rows,
                          hipStream_t stream, uint32_t tile_wlog, rg_stats *stats, rg_pass_launch launch,
                          const void *payload) {
    rg_launch_ctx *cx = rg_ctx_for(s, stream);
    if (!cx) return RG_ERR_OUT_OF_MEMORY;
    s->last = cx;
    RgKernelArgs a = rg_frame_args(s, cx, W, H, t, 1u, rows);
    a.tile_wlog = tile_wlog;
    cx->last_counters = a.counters;
    cx->last_plain = 0;
    cx->last_shvol = 0;
    if (stats && !ok(hipEventRecord(cx->ev0, stream))) return RG_ERR_DEVICE;
    if (rows > 0) {
        if (!ok(launch(&a, payload, stream))) return RG_ERR_DEVICE;
        cx->cur = 1 - cx->cur;  // the kernel zeroes the other set for the next launch
    }
    if (!stats) return RG_OK;
    if (!ok(hipEventRecord(cx->ev1, stream))) return RG_ERR_DEVICE;
    return stats_tail(cx, stream, stats);
}

hipError_t rg_pass_grid(const RgKernelArgs &a, unsigned block, unsigned blocks_per_cu, dim3 *grid, size_t *lds) {
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    const unsigned long long ntiles = rg_tile_count(a), per_block = block / 64u;
    const unsigned long long want = (ntiles + per_block - 1ull) / per_block;
    const unsigned long long cap = (unsigned long long)(cus > 0 ? cus : 1) * blocks_per_cu;
    *grid = dim3((unsigned)(want < cap ? want : cap));
    // per-lane walk stacks (stride = block size): lane_stack entries + the spare slot (rg_k_bvh.h bvh_lane)
    *lds = a.lane_stack > 0 ? ((size_t)(a.lane_stack + 1) * 4u) * block : 0u;
    return hipSuccess;
}

rg_status rg_launch_tiles(const rg_scene *s, const rg_launch_desc &d, rg_launch_ctx **ctx_out) {
    uint32_t out_rows = 0;
    rg_status st = validate(s, d, &out_rows);
    if (st != RG_OK) return st;
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    rg_launch_ctx *cx = rg_ctx_for(s, d.stream);
    if (!cx) return RG_ERR_OUT_OF_MEMORY;
    s->last = cx;
    if (ctx_out) *ctx_out = cx;
    RgKernelArgs a = fill_args(s, d, cx, out_rows);
    const int frames = frames_needed(s->max_depth);
    // host-frame launches of heavy-path scenes run array-frame kernels with the
    // host-frame features (rg_render_kernel.h HF) up to rg_host_array_frames() frames;
    // the others the MAXD == 0 kernels, whose frames live in a global buffer
    const bool host_arrays = frames <= rg_host_array_frames() && rg_heavy_path(a);
    // (so do sparse launches: the SPARSE instantiations exist for MAXD == 0 only; camera launches
    // keep their frames there whatever `disp` says: rg_launch_global_frames)
    const int disp = ((d.host_frame && !host_arrays) || d.px_mask) ? std::max(frames, rg_max_array_frames() + 1) : frames;
    if ((st = size_deep_frames(cx, a, frames, disp)) != RG_OK) return st;
    if ((st = refresh_prim_table(cx, a, d.stream)) != RG_OK) return st;
    if (!rg_heavy_path(a)) {  // light path: one staging loop per block
        a.lds_blob = rg_lds_blob_for(s, a);
        if (!a.lds_blob) a.plain_veto |= 2u;  // the PLAIN kernels' two tables exist in the image only
    }
    if (a.area_tab) {
        // No light buffers: a light's grid is exact for rays towards the light's own position only, and each
        // sample sees the light elsewhere, so shadow rays walk the BVH; the camera buffer goes with them.
        // (After the arena's image is made: its layout and content are the scene's, whatever this launch reads.)
        a.lbuf = nullptr;
        a.lb_start = a.lb_ent = nullptr;
        a.n_lbuf = 0;
        a.lb_cam = -1;
    }
    if (d.timed && !ok(hipEventRecord(cx->ev0, d.stream))) return RG_ERR_DEVICE;  // kernel_ms includes the tile probe
    // a sparse launch's list only schedules: no probe, and the cached order and its key stay as they are
    if (!d.px_mask && (st = order_tiles(s, d, cx, a)) != RG_OK) return st;
    return launch_and_snapshot(d, cx, a, disp);
}

rg_status rg_snap_status(const unsigned long long *snap, rg_stats *stats) {
    if (stats) {
        stats->rays.primary = snap[0];
        stats->rays.shadow = snap[1];
        stats->rays.secondary = snap[2];
        stats->error_pixel = -1;
    }
    return decode_error(snap[3], stats ? &stats->error_pixel : nullptr);
}

extern "C" {

uint32_t rg_tiling_rows(uint32_t height, const rg_tiling *t) { return rg_tiling_rows_grouped(height, t, 1); }

rg_status rg_scene_release_stream(rg_scene *s, void *stream) {
    if (!s) return RG_ERR_INVALID_ARGUMENT;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    if (!hs) return RG_OK;  // the null-stream context lives as long as the scene
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    rg_ambient_release(s, hs, false);
    for (size_t i = 0; i < s->ctxs.size(); ++i) {
        if (s->ctxs[i]->stream != hs) continue;
        rg_launch_ctx *c = s->ctxs[i];
        (void)hipStreamSynchronize(hs);
        if (s->last == c) s->last = rg_ctx_for(s, nullptr);
        s->ctxs.erase(s->ctxs.begin() + (std::ptrdiff_t)i);
        rg_ctx_destroy(c);
        break;
    }
    return RG_OK;
}

rg_status rg_stream_status(const rg_scene *s, void *stream, int32_t *error_pixel) {
    if (!s) return RG_ERR_INVALID_ARGUMENT;
    if (error_pixel) *error_pixel = -1;
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    for (rg_launch_ctx *c : s->ctxs) {
        if (c->stream != hs) continue;
        unsigned long long w = 0;
        if (!ok(hipStreamSynchronize(hs)) || !ok(hipMemcpy(&w, c->sticky, sizeof w, hipMemcpyDeviceToHost)) ||
            !ok(hipMemset(c->sticky, 0, sizeof w)))
            return RG_ERR_DEVICE;
        return decode_error(w, error_pixel);
    }
    return RG_OK;  // nothing was launched on this stream
}

rg_status rg_render_tiles_async(const rg_scene *s, uint32_t width, uint32_t height, const rg_tiling *tiling,
                                uint8_t *rgba_dev, float *rgb_dev, void *stream, rg_stats *stats) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    rg_launch_ctx *cx = nullptr;
    rg_launch_desc d = device_frame(width, height, tiling, rgba_dev, rgb_dev, st);
    d.timed = stats != nullptr;
    rg_status r = rg_launch_tiles(s, d, &cx);
    if (r != RG_OK || !stats) return r;
    return stats_tail(cx, st, stats);
}

rg_status rg_render_tiles_pipelined(const rg_scene *s, uint32_t width, uint32_t height, const rg_tiling *tiling,
                                    uint8_t *rgba_dev, float *rgb_dev, void *stream) {
    // one of several frames in flight (rg_frames, bench.py): the heavy path sizes
    // its grid for throughput (rg_render_grid.h, RgKernelArgs::pipelined)
    rg_launch_desc d = device_frame(width, height, tiling, rgba_dev, rgb_dev, static_cast<hipStream_t>(stream));
    d.pipelined = true;
    return rg_launch_tiles(s, d);
}

}  // extern "C"
