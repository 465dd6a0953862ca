/*
 * raingun_debug.h — test/diagnostic entry points of libraingun_hip.so.
 * Not part of the reference's interface; used by tests/ to exercise every
 * kernel path on every scene.
 */
#ifndef RAINGUN_DEBUG_H
#define RAINGUN_DEBUG_H

#include "raingun.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Force the kernel path used for this scene: -1 = automatic (by body count),
 * 0 = light path (2 waves/SIMD, batched shadow rays, exact f64 tests),
 * 1 = heavy path (4 waves/SIMD, one ray per lane, f32 pre-filter + exact f64). */
rg_status rg_debug_set_path(rg_scene *scene, int32_t path);

/* Sphere BVH (built by rg_scene_create for scenes with at
 * least 16 spheres and used by the heavy path and rg_trace).  Disabling it
 * makes every ray scan all spheres; results are identical either way. */
typedef struct rg_bvh_info {
    int32_t built;         /* a BVH exists for this scene */
    int32_t enabled;       /* and is used by the render/trace launches */
    int32_t nodes;         /* 4-wide nodes (128 B each) */
    int32_t leaves;        /* leaves (<= 4 spheres each) */
    int32_t depth;         /* levels */
    float margin;          /* box inflation, scene units */
    float origin_bound;    /* rays with |o_k| above this scan all spheres */
    int32_t lane_stack;    /* per-lane walk: worst-case stack entries per lane */
    int64_t lbuf_bytes;    /* shadow-ray light buffers + camera buffer, device bytes (capped:
                            * RG_LB_TOTAL_WORDS words; lights past the cap keep the BVH walk) */
} rg_bvh_info;
rg_status rg_debug_set_bvh(rg_scene *scene, int32_t enable);
rg_status rg_debug_bvh_info(const rg_scene *scene, rg_bvh_info *info);

/* Shadow-ray light buffers (heavy path, BVH scenes; rg_lightbuf.cpp): per light,
 * a grid whose cells list every sphere a shadow ray starting there could hit,
 * so a shadow ray tests its cell's spheres instead of walking the BVH.  enable
 * 1 (default) / 0 (the BVH walk for every shadow ray); results are identical
 * either way.  rg_debug_lightbuf_count: lights whose buffer is in use (0 when
 * none was built, the BVH is off, or the buffers are switched off). */
rg_status rg_debug_set_lightbuf(rg_scene *scene, int32_t enable);
int32_t rg_debug_lightbuf_count(const rg_scene *scene);

/* BVH walk per ray kind: rays at recursion depth >= min_depth (secondary rays
 * and the shadow rays of their hits: incoherent) walk the tree per lane with a
 * nearest-first stack; shallower rays walk it wave-coherently.  0 = every
 * non-primary ray per lane, a large value = wave-coherent only, -1 = default
 * (1).  Heavy path only; results are identical either way. */
rg_status rg_debug_set_lane_depth(rg_scene *scene, int32_t min_depth);

/* Tile scheduling: 1 = a primary-ray probe orders each frame's 8x8 tiles by
 * estimated cost, most expensive first (stable within a cost class);
 * 0 = raster order; -1 (default) = ordered on the heavy (trace-dominated)
 * path only.  Results are identical either way. */
rg_status rg_debug_set_tile_order(rg_scene *scene, int32_t mode);

/* Host-visible frames (rg_render_image / rg_render_tiles without f32 RGB):
 * -1 = ONE launch whose pixel stores go over PCIe straight into page-locked
 * host memory (the caller's, or a pinned frame copied band by band into a
 * pageable caller buffer as the kernel publishes finished tiles);
 * 1..16 = render in this many row bands into device memory, each band's
 * device-to-host copy overlapping the next bands' renders; -2 = split (below);
 * 0 (default) = into page-locked buffers: split for light-path scenes, one
 * launch for heavy-path scenes; into pageable buffers: bands (~2 Mpx each, at
 * most 3).  Results are identical for every value. */
rg_status rg_debug_set_image_bands(rg_scene *scene, int32_t bands);

/* bands = -2 (page-locked whole-frame renders; otherwise as -1): the frame in two
 * concurrent parts sharing the PCIe link -- the top `pct` percent of the rows
 * rendered into device memory and copied by DMA, the rest in one launch writing
 * host memory.  pct 1..99, 0 = the library default.  Results are identical. */
rg_status rg_debug_set_host_split(rg_scene *scene, int32_t pct);

/* Fault injection for the split path's error exits: the next `count` split renders
 * report part A's launch as failed (RG_ERR_DEVICE) after part B -- the launch
 * storing into the caller's buffer -- is already enqueued.  The call must still
 * return only once nothing writes that buffer any more.  0 = off (default). */
rg_status rg_debug_fail_split_a(rg_scene *scene, int32_t count);

/* Light-path frames into page-locked host memory (the one-launch host-frame kernels; -1 keeps a
 * setting): finished tiles per LDS-ring flush (1..16, 0 = 16) and consecutive tiles the tile
 * queue hands a wave at a time (0 = the flush size), for launches below 50,000 tiles (`_small`:
 * rg_render_multi's device shares) and from it (`_big`: whole frames);
 * `multi_light_one` 1 (default) = rg_render_multi's automatic mode renders a light scene's device
 * shares as one launch each, 0 = bands + DMA copies.  Results are identical for every setting. */
rg_status rg_debug_set_host_ring(rg_scene *scene, int32_t flush_small, int32_t group_small, int32_t flush_big,
                                 int32_t group_big, int32_t multi_light_one);

/* Tile shape of the one-launch host-visible path: log2 of the tile width,
 * 3 (8x8) .. 6 (64x1), every tile 64 pixels; wider tiles give whole row
 * segments per PCIe write.  0 = automatic (the default: 16x4 for heavy-path
 * scenes, 64x1 for light-path scenes).  Device-resident renders always use 8x8. */
rg_status rg_debug_set_host_tile_shape(rg_scene *scene, int32_t tile_wlog);

/* Supersampled frames (rg_render_image_aa / rg_render_aa_async) render and resolve in
 * bands of `rows` output rows (samples * rows sample rows); 0 (default) = automatic: the
 * band whose samples (16 B each) fit 64 MiB, a multiple of 8 rows, at least 8.  Tests force
 * small bands so that small frames span several.  Results are identical for every value. */
rg_status rg_debug_set_aa_band_rows(rg_scene *scene, int32_t rows);

/* Adaptive anti-aliasing (rg_render_image_aa_adaptive / rg_render_aa_adaptive), a probe for
 * scripts/aa_adaptive_bench.py.  rg_debug_set_aa_adaptive_timing(enable != 0): the following
 * calls record HIP events around their passes.  rg_debug_aa_adaptive_info, of the scene's
 * latest call that ran the passes (threshold >= 1): ms[0] the 1-sample frame, ms[1] the mask
 * kernel, ms[2] the tile-list kernel, ms[3] the sparse renders and ms[4] the adaptive resolves,
 * each summed over the bands (bands on the two render streams overlap, so the sums may exceed
 * the call's span; all zero without timing); *flagged the flagged pixels, *listed_tiles the
 * sample tiles launched, *bands_launched the bands that had any.  Every pointer nullable. */
rg_status rg_debug_set_aa_adaptive_timing(rg_scene *scene, int32_t enable);
rg_status rg_debug_aa_adaptive_info(const rg_scene *scene, float ms[5], uint32_t *flagged, uint32_t *listed_tiles,
                                    uint32_t *bands_launched);

/* rg_render_multi: mode 0 (default) = every device delivers its rows of the
 * frame to the host buffer itself, over its own PCIe link: `bands` = -1 one
 * launch per device whose kernel stores its rows straight into a page-locked
 * frame, 1..4 row bands per device, each band's rows copied while the later
 * bands render, 0 = automatic (one launch for heavy-path scenes into a
 * page-locked frame, else bands); mode 1 = ONE RCCL ncclGather of the parts to the scene's device,
 * re-interleave there, one copy to the host.  stand_in = 1 places every
 * "device" on the scene's device (a replica each) and routes mode 1's gather
 * through a stand-in with ncclGather's signature and group semantics, so
 * ngpus > 1 runs on one GPU (tests).  Results are identical for every setting.
 * only_rank >= 0 (stand-in, mode 0 only) issues only that device's work -- its
 * banded render and its rows' copies to the host -- so one GPU times the
 * timeline one device of an N-GPU node runs (the frame is then incomplete);
 * -1 = every device. */
rg_status rg_debug_set_multi(rg_scene *scene, int32_t mode, int32_t stand_in, int32_t bands, int32_t only_rank);

/* An rg_gather_fn (raingun_frames.h) that does nothing and returns 0: the
 * frame loop's own host cost per frame without a collective (probes). */
int rg_debug_gather_noop(const void *send, void *recv, size_t count, int datatype, int root, void *comm,
                         void *stream);

/* Copy the scene's 16 statistics words after the last render: [0..2] ray
 * counts, [4..8] BVH traversal statistics when the library was built with
 * -DRG_BVH_STATS (zero otherwise). */
rg_status rg_debug_counters(const rg_scene *scene, uint64_t out[16]);

/* Words [first, first + n) of the last render's counter set (RG_COUNTER_WORDS words):
 * diagnostic builds' extra statistics, e.g. -DRG_REGION_STATS region visits at 144.. */
rg_status rg_debug_counter_words(const rg_scene *scene, int32_t first, int32_t n, uint64_t *out);

/* Which light kernel the scene's latest render launch ran: *plain = 1 for the PLAIN instantiation
 * (device-resident light launches of scenes with no disks and no boxes, no f32 RGB output, no
 * tile order, no NaN-scene path and 1..3 lights: those facts are compiled in), 0 for any other
 * kernel.  A word the launcher writes; results are identical either way. */
rg_status rg_debug_last_plain(const rg_scene *scene, int32_t *plain);

/* Shadow mask volume of the PLAIN light kernels (rg_shadow_vol.cpp): a grid over the scene, built by
 * rg_scene_create for scenes of spheres and planes only (1..16 bodies of each kind at most, 1..3
 * lights, every parameter finite and at most 2^20 in magnitude), whose cells name the bodies that
 * could occlude a light from a shadow origin there; a wave tests only the bodies its lanes' cells
 * name.  rg_debug_set_shadow_volume(0): the scene's launches pass no volume and test every body
 * (1, the default: the volume where one was built).  Results are identical either way.
 * rg_debug_shadow_volume_info: whether a volume was built and is switched on, its cells per axis,
 * device bytes, build time on the host and the share of set bits (set / (cells x bodies)).
 * rg_debug_last_shadow_volume: *used = 1 if the scene's latest render launch ran a PLAIN kernel
 * with the volume, else 0. */
typedef struct rg_shadow_volume_info {
    int32_t built;
    int32_t enabled;
    int32_t g;
    int32_t pad;
    int64_t bytes;
    double build_ms;
    double set_share;
} rg_shadow_volume_info;
rg_status rg_debug_set_shadow_volume(rg_scene *scene, int32_t on);
rg_status rg_debug_shadow_volume_info(const rg_scene *scene, rg_shadow_volume_info *info);
rg_status rg_debug_last_shadow_volume(const rg_scene *scene, int32_t *used);

/* First-hit tiles of the PLAIN light kernels: an 8x8 tile whose 64 primary rays all end at a miss, a
 * diffuse hit, or a reflecting hit at the depth limit needs no recursion state, and its wave shades
 * and stores it in one straight line (primary hit, shadow batch, shade, store) instead of three trips
 * round the general state machine; any other tile, and any tile with a shadow ray that could see a NaN
 * distance, goes the general way.  rg_debug_set_first_hit_tiles(0): no tile of the scene's launches
 * takes the path (1, the default: the wave's vote decides).  Results are identical either way.
 * rg_debug_last_first_hit_tiles: *tiles = the tiles of the scene's latest render launch that finished
 * on the path (0 for any other kernel). */
rg_status rg_debug_set_first_hit_tiles(rg_scene *scene, int32_t on);
rg_status rg_debug_last_first_hit_tiles(const rg_scene *scene, uint64_t *tiles);

/* The PLAIN light kernels compute the camera ray's two quotients from host reciprocals and its
 * length without range scaling, after the launcher has checked the frame size column by column and
 * row by row and bounded the field of view.  rg_debug_set_exact_div(0): the scene's launches behave
 * as if that check had failed, so they run the general kernel (1, the default: the check decides).
 * Results are identical either way.
 * rg_debug_camera_check: a small kernel computes the camera direction of every pixel of a
 * width x height frame at `fov` degrees both ways; *mismatches = the pixels whose directions
 * differ in any bit, *admitted (nullable) = 1 if the launcher's checks admit that frame, else 0. */
rg_status rg_debug_set_exact_div(rg_scene *scene, int32_t enable);
rg_status rg_debug_camera_check(const rg_scene *scene, uint32_t width, uint32_t height, double fov,
                                uint64_t *mismatches, int32_t *admitted);

/* The PLAIN light kernels take ONE f64 square root and reciprocal -- a spherical light's distance
 * and 1 / distance at every shaded hit -- without the range scaling around them, in every lane whose
 * operand's exponent lies in a window around 1 (biased exponent 767..1279); the other lanes of such a
 * wave take the compiler's own sqrt and division.  Every other sqrt and division of those kernels is
 * the compiler's.  rg_debug_unscaled_check runs the guarded primitives on the device for n
 * caller-supplied operands (n <= 2^24) --
 * op 3: sqrt(a[i]) and 1.0 / sqrt(a[i]) from one admission, the form the kernels run;
 * op 0: sqrt(a[i]); 1: 1.0 / a[i]; 2: a[i] / b[i] (b is read by op 2 only): the same scheme for a
 * lone root, reciprocal and quotient, which no render kernel runs (they measured slower there) --
 * and beside them the compiler's operations; *mismatches = the operands whose results differ in any bit. */
rg_status rg_debug_unscaled_check(const rg_scene *scene, int32_t op, const double *a, const double *b, uint32_t n,
                                  uint64_t *mismatches);

#ifdef __cplusplus
}
#endif

#endif /* RAINGUN_DEBUG_H */
