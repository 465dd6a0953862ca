// rg_internal.h — host-side state behind the opaque rg_scene handle (what the description
// determines is in rg_scene_tables.h, built without a device by rg_scene_build.cpp), shared
// by rg_scene.hip (scene upload, replicas, kernel arguments), rg_launch.hip (per-stream
// launch contexts, the tiled launch, the launch path of the pixel passes: rg_frame_args,
// rg_pass_check / rg_pass_enqueue, rg_pass_grid), rg_capi.hip (host-visible frames,
// streaming, debug setters), rg_aa.hip (supersampled frames and their adaptive form),
// rg_aov.hip (the AOV pass), rg_ao.hip (the ambient occlusion pass), rg_ambient.hip (the
// ambient term), rg_frames.hip (frames in flight over N processes), rg_multi.hip (one process driving N
// devices), rg_gather.hip (the pack and re-interleave kernels of both) and rg_rccl.hip
// (the run-time RCCL loader, rg_rccl.h, and the rg_comm_* functions).  The band resource
// set the two kinds of host frames are built on is in rg_bands.h, the band arithmetic in
// rg_band_plan.h, the dealing of tiles to ranks and devices in rg_tile_deal.h, the merge of
// per-pass statistics in rg_stats_merge.h.  Defined here: rg_scratch (the device scratch of a
// blocking entry) and rg_table_once (a device table made once per scene).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <vector>

#include "../../include/raingun.h"
#include "../../include/raingun_debug.h"
#include "rg_bands.h"
#include "rg_copy_pool.h"
#include "rg_device.h"
#include "rg_lightbuf_ray.h"
#include "rg_scene_tables.h"
#include "rg_stats_merge.h"
#include "rg_tile_deal.h"

inline bool ok(hipError_t e) { return e == hipSuccess; }

// Per-stream launch state (ray counters, tile-queue heads, error words, tile
// ordering scratch, deep frame buffer, timing events).  Launches on distinct
// streams may run concurrently (frames in flight), so they must not share it;
// launches on one stream are ordered by the stream and reuse it.
struct rg_launch_ctx {
    hipStream_t stream = nullptr;
    // Two sets of RG_COUNTER_WORDS words (rg_device.h), used by alternate
    // launches: a render kernel counts into set `cur` and zeroes the other set
    // (the previous launch's, already read back: same stream), so the next
    // launch finds its set zeroed without a memset of its own.
    unsigned long long *counters = nullptr;
    int cur = 0;
    unsigned long long *last_counters = nullptr;  // the set of the latest launch (rg_debug_counters)
    int last_plain = 0;  // the latest launch ran a PLAIN light kernel (rg_debug_last_plain)
    int last_shvol = 0;  // ... with the scene's shadow mask volume (rg_debug_last_shadow_volume)
    unsigned long long *sticky = nullptr;    // first error of any launch since rg_stream_status cleared it
    uint32_t *tile_cost = nullptr, *tile_perm = nullptr;  // probe/sort scratch (rg_launch_tile_order), order
    size_t tile_cap = 0;
    // the launch the cached tile_perm was made for: the order is a function of
    // the frame geometry and the scene (probe rays, materials, lights, depth)
    struct PermKey {
        uint32_t width, height, tile_rows, tile_stride, tile_offset, tile_base, out_rows, tile_wlog, max_depth, n_lights,
            tile_group;
        double fov;
        const void *mats;
        bool camera = false;  // the launch's camera (RgKernelArgs::camera, cam_eye .. cam_forward), zero without one
        double cam[12] = {};
        bool operator==(const PermKey &o) const {
            if (camera != o.camera || std::memcmp(cam, o.cam, sizeof cam) != 0) return false;
            return width == o.width && height == o.height && tile_rows == o.tile_rows && tile_stride == o.tile_stride &&
                   tile_offset == o.tile_offset && tile_base == o.tile_base && out_rows == o.out_rows &&
                   tile_group == o.tile_group &&
                   tile_wlog == o.tile_wlog && max_depth == o.max_depth &&
                   n_lights == o.n_lights && fov == o.fov && mats == o.mats;
        }
    };
    bool perm_valid = false;
    PermKey perm_key{};
    void *deep = nullptr;  // frames for depths above the compiled arrays (rg_k_frames.h FrameStack<0>)
    size_t deep_bytes = 0;
    double *prim = nullptr;  // sensor x per column then sensor y per row (RgKernelArgs::prim_sx / prim_sy)
    size_t prim_cap = 0;     // bytes
    uint32_t prim_w = 0, prim_h = 0;
    double prim_fov = 0.0;
    // the frame size whose camera quotients were last swept (rg_exact.h rg_recip_div_ok), and the verdict
    uint32_t rdiv_w = 0, rdiv_h = 0;
    bool rdiv_ok = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

#ifndef RG_IMAGE_STREAM_CUMASK
#define RG_IMAGE_STREAM_CUMASK 1  // host-frame render streams with a CU mask: a hardware queue each (rg_capi.hip)
#endif
#ifndef RG_HOST_TILE_WLOG_LIGHT
// one-launch host-visible frames of light-path scenes: 64x1 tiles, so that a wave's ring of
// consecutive tiles (rg_render_cfg.h RG_HOST_RING) is one contiguous run of host memory
#define RG_HOST_TILE_WLOG_LIGHT 6
#endif
#ifndef RG_HOST_TILE_WLOG
// one-launch host-visible frames of heavy-path scenes: 16x4 tiles (RgKernelArgs::tile_wlog) --
// 64-B row segments per PCIe write, where 8x8 tiles send 32-B ones and 64x1 tiles lose the BVH
// walk's coherence: north star into pinned memory 2.53 -> 2.14 ms (8x8 -> 16x4; 32x2 2.22,
// 64x1 2.66: profiles/r05/s13, s14, s15)
#define RG_HOST_TILE_WLOG 4
#endif
// Resources of the host-visible paths (rg_render_image / rg_render_tiles /
// rg_render_stream), owned by the scene and reused across calls: a band resource set
// (rg_bands.h) whose rs[1] has a hardware queue of its own, and what the one-launch
// paths need.
struct rg_image_res : rg_band_res {
    void *h_frame = nullptr;  // pinned, coherent: whole frames the kernel writes over PCIe (pageable destinations)
    size_t h_frame_cap = 0;
    uint32_t *h_flags = nullptr;  // pinned, coherent: per-tile publication words (RgKernelArgs::tile_flags)
    size_t h_flags_cap = 0;       // bytes
    uint32_t seq = 0;             // frame sequence number the flags carry
    uint32_t *h_cancel = nullptr; // pinned, coherent: streaming cancellation word (RgKernelArgs::cancel)
};

#define RG_AA_MAX_SAMPLES 8  // samples per pixel side
// Resources of the supersampled paths (rg_render_image_aa / rg_render_aa_async), owned by
// the scene and reused across calls: a band resource set of plain streams (render + resolve
// on rs, d_rgba / d_rgb the resolved frame of the host entry), and the sample scratch.
struct rg_aa_res : rg_band_res {
    hipEvent_t ev_fork = nullptr;  // rg_render_aa_async: the caller's stream
    // per render stream, one band of samples: RGBA8 (the render kernel always writes it) and f32 RGB
    void *slot_rgba[2] = {nullptr, nullptr};
    void *slot_rgb[2] = {nullptr, nullptr};
    size_t slot_cap[2] = {0, 0};  // samples
    // adaptive anti-aliasing (rg_render_image_aa_adaptive / rg_render_aa_adaptive): the 1-sample
    // pass, the mask and the tile lists run on a stream of their own (a launch context, so a
    // primary-ray table and a tile order, of the W x H frame beside the bands' of the sample frame)
    hipStream_t base_stream = nullptr;
    hipEvent_t ev_list = nullptr;  // the base frame, the mask and the lists are made
    uint8_t *d_mask = nullptr;     // W x H bytes (when the caller gives no mask buffer)
    size_t d_mask_cap = 0;
    uint32_t *d_list = nullptr;    // per band, the listed sample tiles (bands x tiles of a full band)
    size_t d_list_cap = 0;         // bytes
    uint32_t *d_counts = nullptr;  // per band its listed tiles, then the mask kernel's sharded flagged counters
    size_t d_counts_cap = 0;       // bytes
    uint32_t *h_counts = nullptr;  // pinned: the same, read between the passes
    size_t h_counts_cap = 0;       // bytes
    // the probe of include/raingun_debug.h (rg_debug_set_aa_adaptive_timing / rg_debug_aa_adaptive_info)
    bool timing = false;
    std::vector<hipEvent_t> ev_mark;  // timing events, in the order the passes record them
    size_t n_marks = 0;
    float pass_ms[5] = {0, 0, 0, 0, 0};
    uint32_t flagged = 0, listed_tiles = 0, bands_launched = 0;
    // the thin lens's tables on the device (rg_lens.h RG_LENS_TABLE_DOUBLES doubles): made on the first frame
    // through a lens (rg_table_once), never rewritten, so launches in flight may read them whatever the scene
    // is given next
    double *d_lens = nullptr;
};

// Resources of the ambient frames (rg_render_ambient_async, rg_ambient.hip), one set per stream used: the layers
// between the passes (f32 rgb, albedo, normal; body; the raw and the filtered AO pass) in one allocation, and
// the events around the two image kernels.
struct rg_ambient_res {
    hipStream_t stream = nullptr;
    void *mem = nullptr;
    size_t cap = 0;  // bytes
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

struct rg_multi_res;  // rg_multi.hip
struct rg_frames;     // rg_frames.hip (include/raingun_frames.h)

// What the setters change after creation and a launch reads.  A replica on another device follows
// its root scene's, whole, before every frame (rg_sync_settings): a member added here is synced.
struct rg_scene_settings {
    uint32_t max_depth = 10;
    int32_t path = RG_PATH_AUTO;
    int32_t lane_min_depth = 1;  // rays of this depth and deeper walk the BVH per lane
    bool bvh_enabled = true;
    bool lbuf_enabled = true;       // rg_debug_set_lightbuf
    bool shvol_enabled = true;      // rg_debug_set_shadow_volume
    bool first_hit_enabled = true;  // rg_debug_set_first_hit_tiles
    bool exact_div = true;          // rg_debug_set_exact_div: 0 = launches behave as if the quotient sweep had failed
    // rg_scene_set_camera: host state, read when a launch is enqueued and passed by value in its kernel
    // arguments (RgKernelArgs::camera ..), so launches in flight keep the camera they were enqueued with
    bool has_camera = false;
    rg_camera camera{};
    // rg_scene_set_lens: host state like the camera, read when a band of a supersampled frame is enqueued
    // and passed by value (RgKernelArgs::lens ..); aperture == 0: no lens
    rg_lens lens{0.0, 1.0};
    // rg_scene_set_light_radii (rg_area.h): one radius per light (empty: point lights) and whether any is > 0;
    // the device table made from them is rg_scene::d_area
    std::vector<double> light_radii;
    bool area_any = false;
    int tile_order = -1;  // expensive tiles first (rg_tile_order.hip "tile ordering"): -1 auto (heavy path), 0, 1
    // light-path host frames (rg_debug_set_host_ring): LDS-ring flush size and queue group of small
    // (< RG_RING_BIG_TILES tiles) and big launches
    int ring_flush_small = RG_RING_FLUSH_SMALL, ring_group_small = RG_RING_GROUP_SMALL;
    int ring_flush_big = RG_RING_FLUSH_BIG, ring_group_big = RG_RING_GROUP_BIG;
};

// A scene on one device.  Four kinds of state (DESIGN.md "Scene state"): the facts the description
// determines (rg_scene_facts, rg_scene_tables.h) and the settings, both inherited so that their
// members read s->n_sph, s->camera; the device tables; and the resources launches reuse.
struct rg_scene : rg_scene_facts, rg_scene_settings {
    int device = 0;
    // device tables: the host tables (host, shared with the replicas) uploaded to this device
    std::shared_ptr<const rg_host_tables> host;
    mutable std::vector<void *> allocations;  // freed with the scene: the tables below and rg_table_once's
    RgSph *sph = nullptr;
    double *sph_cc = nullptr;
    RgSphF *sphf = nullptr;
    RgSphF2 *sphf2 = nullptr;
    int32_t *sph_id = nullptr, *pln_id = nullptr, *dsk_id = nullptr, *box_id = nullptr;
    RgPln *pln = nullptr;
    RgDsk *dsk = nullptr;
    RgBox *box = nullptr;
    RgBodyDev *bodies = nullptr;
    RgMatDev *mats = nullptr;
    RgLightDev *lights = nullptr;
    RgTexDev *texs = nullptr;
    RgBvhNode *nodes = nullptr;     // sphere BVH (sphere tables are in its leaf order)
    RgLightBufDev *lbuf = nullptr;  // shadow-ray light buffers (rg_lightbuf.cpp), n_lbuf lights
    uint32_t *lb_start = nullptr, *lb_ent = nullptr;
    uint32_t *shvol = nullptr;      // shadow mask volume of the PLAIN light kernels (rg_shadow_vol.cpp), null: none
    std::vector<RgTexDev> tex_desc;  // the uploaded texture descriptors (device texel pointers)
    // the LDS arena as one device image (RgKernelArgs::lds_blob), and the layout it was built for
    void *lds_blob = nullptr;
    rg_lds_layout lds_blob_layout{};
    // The device table of the settings' light radii, which a band of a supersampled frame reads them from
    // (RgKernelArgs::area_tab: every k's points, then the radii).  Unlike the camera and the lens the radii
    // are as many as the scene has lights, so they travel by reference: the table is rewritten only with the
    // device idle (rg_area_upload).  area_stale: the host radii are newer than the table (a replica, whose
    // table is made when a frame first needs it).
    bool area_stale = false;
    double *d_area = nullptr;
    // the ambient occlusion pass's table on the device (rg_ao.h RG_AO_TABLE_DOUBLES doubles: every k's points,
    // then the lens's rotations): made on the first AO frame (rg_ao.hip, rg_table_once), never rewritten
    mutable double *d_ao = nullptr;
    // the ambient term's share per body on the device (host->amb_share): made on the first ambient frame
    // (rg_ambient.hip, rg_table_once), never rewritten
    mutable float *d_share = nullptr;
    // Settings of the host-visible and multi-device paths, read on the root scene only (not synced to replicas):
    int image_bands = 0;  // host-visible frames: 0 auto, -1 one launch writing host memory, -2 split, 1..16 row bands
    int host_split_pct = 0;  // -2 (split): percent of the frame's rows rendered into device memory + DMA (0: default)
    mutable int split_fail_a = 0;  // debug: the next N split renders report part A's launch as failed (rg_debug_fail_split_a)
    // rg_render_multi's automatic mode renders each light-scene device share as one launch (else bands + DMA)
    bool multi_light_one = RG_MULTI_LIGHT_ONE != 0;
    int host_tile_wlog = RG_HOST_TILE_WLOG;  // tile shape of the one-launch host-visible path
    bool host_tile_forced = false;           // set by rg_debug_set_host_tile_shape (else light scenes: 64x1)
    // rg_render_multi (rg_debug_set_multi): 0 each device copies its rows to the host, 1 RCCL gather;
    // stand-in: every "device" is this one, gathers through a stand-in (tests on one GPU);
    // bands per device share in the direct mode (0: automatic)
    int multi_mode = 0;
    bool multi_stand_in = false;
    int multi_bands = 0;
    int multi_only_rank = -1;  // stand-in direct mode: issue only this device's work (timeline rehearsal)
    int aa_band_rows = 0;  // supersampled frames: output rows per band (rg_debug_set_aa_band_rows), 0 automatic
    // resources, made on first use and reused across calls
    mutable std::vector<rg_launch_ctx *> ctxs;  // one per stream used
    mutable rg_launch_ctx *last = nullptr;       // the context of the latest launch (rg_debug_counters)
    mutable rg_image_res img;
    mutable rg_aa_res aa;
    mutable std::vector<rg_ambient_res> amb;  // one per stream used
    mutable rg_multi_res *multi = nullptr;
    // frame pipelines built on this scene: a scene destroyed first detaches them
    // (rg_frames_destroy then no longer touches it), in either destruction order
    mutable std::vector<rg_frames *> frames;
};

// rg_frames.hip: the scene of `f` is going away (rg_scene_destroy)
void rg_frames_detach_scene(rg_frames *f);

// Kernel arguments of a scene (tables, LDS arena, frame constants).
RgKernelArgs rg_make_args(const rg_scene *s);

// One tiled render (rg_launch_tiles); the member initialisers are the defaults.
struct rg_launch_desc {
    uint32_t width = 0, height = 0;
    rg_tiling tiling{};
    uint8_t *rgba = nullptr;  // device memory, or page-locked host memory when host_frame
    float *rgb = nullptr;     // nullable
    hipStream_t stream = nullptr;
    // nullable, host memory, pinned for a truly asynchronous copy: the launch's 4 counter
    // words (rays by class, error key) are copied there after the kernel
    unsigned long long *snap = nullptr;
    bool timed = false;  // record the context's ev0/ev1 around the launch (kernel_ms)
    // per-tile publication words, the sequence number they carry and the cancellation word
    // (RgKernelArgs::tile_flags / frame_seq / cancel), all nullable
    uint32_t *tile_flags = nullptr;
    uint32_t frame_seq = 0;
    const uint32_t *cancel = nullptr;
    uint32_t tile_wlog = 3;   // tile shape (RgKernelArgs::tile_wlog), 3: 8x8
    bool host_frame = false;  // rgba is page-locked host memory
    bool pipelined = false;   // frames in flight: size the grid for throughput
    bool image_rows = false;  // host_frame only: rgba is the whole image, pixels go to their image rows
    // a band of the tiling's selection: selected tiles [tile_first, tile_first + tile_count),
    // rgba / rgb pointing at tile_first's first row
    uint32_t tile_first = 0, tile_count = 0xFFFFFFFFu;
    uint32_t tile_group = 1;  // groups of tile_group consecutive image tiles per stride (RgKernelArgs::tile_group)
    // a sparse launch (px_mask non-null; device-resident 8x8 tiles only): of the launch's tiles only
    // tile_list[0 .. tile_limit) (device memory) are rendered, and of their pixels (x, y) only those with
    // px_mask[(y / px_k) * px_w + x / px_k] != 0 (RgKernelArgs::px_mask); the tiles are not reordered
    const uint32_t *tile_list = nullptr;
    uint32_t tile_limit = 0;
    const uint8_t *px_mask = nullptr;
    uint32_t px_k = 1, px_w = 0;
    // >= 2: a band of a supersampled frame with lens_k x lens_k samples per pixel, which sees the scene's
    // lens if it has one (rg_lens.h rg_lens_active; dense device-resident launches only); lens_tab: the
    // device tables (rg_aa_res::d_lens)
    uint32_t lens_k = 0;
    const double *lens_tab = nullptr;
    // ... and the scene's area lights if any light has a radius (rg_area.h rg_area_active): the scene's device
    // table (rg_scene::d_area); such a launch reads the turns of lens_tab too
    const double *area_tab = nullptr;
};

// Enqueue one tiled render on d.stream (the body of rg_render_tiles_async).
// ctx_out (nullable): the stream's launch context.
rg_status rg_launch_tiles(const rg_scene *s, const rg_launch_desc &d, rg_launch_ctx **ctx_out = nullptr);

// Ray counts and status of a counter snapshot (stats nullable).
rg_status rg_snap_status(const unsigned long long *snap, rg_stats *stats);

// Host-visible render of `tiling` into host buffers (rg_render_tiles / rg_render_image).
rg_status rg_render_host(const rg_scene *s, uint32_t width, uint32_t height, const rg_tiling *tiling,
                         uint8_t *rgba_out, float *rgb_out, rg_stats *stats);

// Is [p, p + bytes) page-locked host memory the DMA engine can write directly?
bool rg_host_is_pinned(const void *p, size_t bytes);
// The device address of page-locked host memory [p, p + bytes) (nullptr: not pinned).
void *rg_host_device_ptr(void *p, size_t bytes);

// A copy of `src` on `device`: its facts, its host tables uploaded there, its settings.
rg_status rg_scene_replica(const rg_scene *src, int32_t device, rg_scene **out);
void rg_scene_free(rg_scene *s);
// dst's settings become src's (every member of rg_scene_settings); changed light radii mark dst's area table stale.
void rg_sync_settings(rg_scene *dst, const rg_scene *src);
// The scene's area table (rg_area.h: the points, then s->light_radii) onto its device, made on first use.
// Blocking: it waits for the device to go idle before it writes, so no launch in flight reads a torn table.
rg_status rg_area_upload(rg_scene *s);

// rg_multi.hip: free the scene's multi-GPU resources (replicas, communicators).
void rg_multi_release(const rg_scene *s);

// Shared between the library's own files only: not exported.
#pragma GCC visibility push(hidden)

// rg_launch.hip: the launch context of `stream`, created on first use (nullptr: out of
// memory / device error), and its destruction.
rg_launch_ctx *rg_ctx_for(const rg_scene *s, hipStream_t stream);
void rg_ctx_destroy(rg_launch_ctx *c);

// Grow-only buffers under one capacity: nothing if want <= cap; else free, null, allocate,
// set the capacity.  RG_MEM_DEVICE: hipMalloc; RG_MEM_PINNED: hipHostMallocDefault;
// RG_MEM_PINNED_ZEROED: hipHostMallocCoherent, zeroed.  clear_error: a failed allocation's
// error is cleared from the runtime (hipGetLastError).
enum rg_mem { RG_MEM_DEVICE, RG_MEM_PINNED, RG_MEM_PINNED_ZEROED };
struct rg_grow_buf {
    void **p;
    size_t bytes;
    template <class T>
    rg_grow_buf(T *&q, size_t n) : p(reinterpret_cast<void **>(&q)), bytes(n) {}
};
rg_status rg_grow(rg_mem kind, size_t &cap, size_t want, std::initializer_list<rg_grow_buf> bufs,
                  bool clear_error = true);
template <class T>
rg_status rg_grow(rg_mem kind, T *&p, size_t &cap, size_t bytes) {  // one buffer, capacity in bytes
    return rg_grow(kind, cap, bytes, {{p, bytes}});
}

// rg_launch.hip: rg_make_args(s) plus what every launch of a frame sets: the context's counter sets (a launch
// counts into set `cur`) and sticky word, the frame and its doubles, the tiling, out_rows, and the scene's camera
// by value (the launch keeps it whatever the scene is given next).  The tile shape and the rest are the caller's.
RgKernelArgs rg_frame_args(const rg_scene *s, rg_launch_ctx *cx, uint32_t W, uint32_t H, const rg_tiling &t,
                           uint32_t tile_group, uint32_t out_rows);

// rg_launch.hip: a pixel pass (one one-shot kernel over the tiles of a tiling: rg_aov.hip, rg_ao.hip) in two
// steps.  rg_pass_check: the frame and the tiling (the first failing check decides the status), *rows = the
// rows the tiling selects, the scene's device made current.  rg_pass_enqueue: the stream's launch context, the
// frame's arguments with `tile_wlog`, launch(&args, payload, stream) unless rows == 0 (then nothing is enqueued
// and the counter sets do not flip), and with `stats` the wait for the launch, its time and its counters
// (without: no synchronisation).
typedef hipError_t (*rg_pass_launch)(const RgKernelArgs *a, const void *payload, hipStream_t stream);
rg_status rg_pass_check(const rg_scene *s, uint32_t W, uint32_t H, const rg_tiling *t, uint32_t *rows);
rg_status rg_pass_enqueue(const rg_scene *s, uint32_t W, uint32_t H, const rg_tiling &t, uint32_t rows,
                          hipStream_t stream, uint32_t tile_wlog, rg_stats *stats, rg_pass_launch launch,
                          const void *payload);
// rg_launch.hip: the one-shot grid of a pixel pass whose waves stride over the launch's tiles: blocks of `block`
// threads (a tile per wave), at most blocks_per_cu per CU of the current device; *lds: the per-lane walk stacks.
hipError_t rg_pass_grid(const RgKernelArgs &a, unsigned block, unsigned blocks_per_cu, dim3 *grid, size_t *lds);

// The device scratch of a blocking entry point: allocate everything, return on status(), run the copies and
// launches; the buffers are freed when the entry returns.  After a failed allocation (RG_ERR_OUT_OF_MEMORY, the
// runtime's last error cleared) dev() allocates nothing more.
class rg_scratch {
    void *buf[8];
    int n = 0;
    rg_status st = RG_OK;

public:
    rg_scratch() = default;
    rg_scratch(const rg_scratch &) = delete;
    rg_scratch &operator=(const rg_scratch &) = delete;
    ~rg_scratch() {
        while (n > 0) (void)hipFree(buf[--n]);
    }
    template <class T>
    T *dev(size_t bytes) {
        void *p = nullptr;
        if (st != RG_OK || n == 8 || !ok(hipMalloc(&p, bytes))) {
            if (st == RG_OK) (void)hipGetLastError();
            st = RG_ERR_OUT_OF_MEMORY;
            return nullptr;
        }
        buf[n++] = p;
        return static_cast<T *>(p);
    }
    rg_status status() const { return st; }
};

// A device table made once per scene and never rewritten, so launches in flight may read it whatever comes next:
// nothing if `slot` is set; else `bytes` of device memory with `host` copied in (blocking: complete before the
// first launch that reads it is enqueued; a null host copies nothing), freed with the scene.
template <class T>
rg_status rg_table_once(const rg_scene *s, T *&slot, const void *host, size_t bytes) {
    if (slot) return RG_OK;
    void *d = nullptr;
    if (!ok(hipMalloc(&d, bytes))) {
        (void)hipGetLastError();
        return RG_ERR_OUT_OF_MEMORY;
    }
    if (host && !ok(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice))) {
        (void)hipFree(d);
        return RG_ERR_DEVICE;
    }
    s->allocations.push_back(d);
    slot = static_cast<T *>(d);
    return RG_OK;
}

// rg_scene.hip: RgKernelArgs::fov_adjustment of a field of view in degrees.
double rg_fov_adjustment(double fov);
// rg_scene.hip: is the scene on the heavy path (rg_device.h rg_heavy_path)?
bool rg_scene_heavy(const rg_scene *s);
// rg_scene.hip: the LDS arena of launch args `a` (made by rg_make_args) as one device image (light
// path: RgKernelArgs::lds_blob), cached per layout; nullptr if it cannot be made.
const void *rg_lds_blob_for(const rg_scene *s, const RgKernelArgs &a);

// rg_capi.hip: tile shape (RgKernelArgs::tile_wlog) of the one-launch host-visible paths.
uint32_t rg_host_tile_wlog(const rg_scene *s);
// rg_capi.hip: free the host-visible paths' resources.
void rg_image_res_release(rg_image_res &r);
// rg_aa.hip: free the supersampled paths' resources.
void rg_aa_res_release(rg_aa_res &r);

// rg_ambient.hip: free the ambient frames' resources of `stream`, or of every stream (all).
void rg_ambient_release(const rg_scene *s, hipStream_t stream, bool all);

// rg_gather.hip: pack npx RGBA pixels to RGB (3 B per pixel), as a part travels in a gather.
hipError_t rg_launch_pack_rgb(const void *rgba, void *rgb, size_t npx, hipStream_t stream);
// rg_gather.hip: the image from the parts of `world` ranks dealt `root` tiles of rank 0 per period
// (rg_tile_deal.h): rank 0's RGBA part read in place, rank r's packed part at gathered + r * slot_bytes.
hipError_t rg_launch_reinterleave(const void *gathered, const void *root_part, void *image, uint32_t width,
                                  uint32_t height, uint32_t tile_rows, uint32_t world, size_t slot_bytes,
                                  hipStream_t stream, uint32_t root = 1);

#pragma GCC visibility pop
