/*
 * raingun.h — C ABI of the MI355X-native renderer for raingun's per-pixel
 * ray-trace path (libraingun_hip.so).
 *
 * The reference has no FFI layer: the seam this ABI replaces is the Rust
 * function
 *     rendering::render_image(scene: &Scene, width: u32, height: u32)
 *         -> ImageBuffer<Rgba<u8>, Vec<u8>>          raingun-lib/src/rendering.rs:24-38
 * reached through Scene::render_image (raingun-lib/src/scene.rs:41-43) from
 * the batch driver (src/render.rs:55).  Everything below that call
 * (render_pixel / get_color / cast_ray / shade_diffuse / fresnel and the body,
 * ray, light, material and colour primitives) runs inside one HIP megakernel
 * for gfx950.
 *
 * All plain C: pointers, sizes, POD structs.  No torch types, no C++.
 * Paths are relative to /root/reference.
 */
#ifndef RAINGUN_H
#define RAINGUN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RG_ABI_VERSION 1

/* ------------------------------------------------------------------------
 * Status codes.  The reference panics; the ABI returns one negative code per
 * panic site instead (no exception or abort ever crosses the boundary).
 * ---------------------------------------------------------------------- */
typedef enum rg_status {
    RG_OK = 0,
    RG_ERR_INVALID_ARGUMENT = -1,   /* null pointers, zero sizes, bad enum values */
    RG_ERR_PORTRAIT = -2,           /* assert!(width >= height)          ray.rs:42 */
    RG_ERR_AABB_NORMAL = -3,        /* "Could not determine normal"       bodies.rs:324 */
    RG_ERR_NAN_DISTANCE = -4,       /* partial_cmp(..).unwrap() on NaN    scene.rs:38 */
    RG_ERR_TRANSMISSION = -5,       /* create_transmission(..).unwrap()   rendering.rs:106 */
    RG_ERR_TEXTURE = -6,            /* texture index out of range / empty image (material.rs:34-47) */
    RG_ERR_DEVICE = -10,            /* HIP runtime error */
    RG_ERR_OUT_OF_MEMORY = -11,
    RG_ERR_CANCELLED = -12,         /* streaming receiver dropped         rendering.rs:53-54 */
    RG_ERR_COLLECTIVE = -13,        /* rg_render_multi: RCCL missing or a collective failed */
    RG_ERR_PENDING = -14            /* rg_frames_read_image: a frame batch still waits for its gather
                                       (call rg_frames_flush on every rank first) */
} rg_status;

/* ------------------------------------------------------------------------
 * Flat POD scene description — mirrors `Scene` (scene.rs:11-19) after serde
 * has run: bodies and lights in YAML order, textures already decoded to RGBA8
 * (material.rs:34-47 decodes eagerly at load time).
 * ---------------------------------------------------------------------- */
enum rg_body_kind {            /* bodies.rs:41-47 */
    RG_BODY_SPHERE = 0,        /* p = {center.x, center.y, center.z, radius}                 */
    RG_BODY_PLANE = 1,         /* p = {origin.x, origin.y, origin.z, normal.x, normal.y, normal.z} */
    RG_BODY_DISK = 2,          /* p = {origin.xyz, normal.xyz, radius}                        */
    RG_BODY_AABB = 3           /* p = {bounds[0].xyz, bounds[1].xyz}                          */
};

enum rg_coloration_kind {      /* material.rs:20-24 */
    RG_COLORATION_COLOR = 0,
    RG_COLORATION_TEXTURE = 1
};

enum rg_surface_kind {         /* material.rs:49-54 */
    RG_SURFACE_DIFFUSE = 0,
    RG_SURFACE_REFLECTING = 1,
    RG_SURFACE_REFRACTIVE = 2
};

enum rg_light_kind {           /* lights.rs:22-26 */
    RG_LIGHT_DIRECTIONAL = 0,  /* v = direction */
    RG_LIGHT_SPHERICAL = 1     /* v = position  */
};

typedef struct rg_material {   /* material.rs:7-12 */
    uint32_t coloration;       /* rg_coloration_kind */
    float color[3];            /* Coloration::Color, f32 RGB in [0,1] (color.rs:7-11) */
    int32_t texture;           /* Coloration::Texture: index into rg_scene_desc.textures */
    float x_offset, y_offset;  /* Texture::{x_offset,y_offset} (material.rs:30-31) */
    float albedo;
    uint32_t surface;          /* rg_surface_kind */
    float reflectivity;        /* Surface::Reflecting */
    float index;               /* Surface::Refractive */
    float transparency;        /* Surface::Refractive */
} rg_material;

typedef struct rg_body {
    uint32_t kind;             /* rg_body_kind */
    uint32_t _pad;
    double p[7];
    rg_material material;
} rg_body;

typedef struct rg_light {      /* lights.rs:8-20 */
    uint32_t kind;             /* rg_light_kind */
    float color[3];
    float intensity;
    uint32_t _pad;
    double v[3];
} rg_light;

typedef struct rg_texture {    /* decoded DynamicImage, RGBA8 row-major, width*height*4 bytes */
    uint32_t width, height;
    const uint8_t *rgba;
} rg_texture;

typedef struct rg_scene_desc { /* scene.rs:11-19; defaults scene.rs:21-31 */
    double fov;                /* degrees, default 90 */
    float default_color[3];    /* default black */
    uint32_t max_recursion_depth; /* default 10 */
    uint32_t n_bodies;
    const rg_body *bodies;
    uint32_t n_lights;
    const rg_light *lights;
    uint32_t n_textures;
    const rg_texture *textures;
} rg_scene_desc;

/* Ray counts by class.  A ray is one Scene::trace call (scene.rs:34-39):
 * primary rendering.rs:73, shadow rendering.rs:150, secondary rendering.rs:126. */
typedef struct rg_ray_counts {
    uint64_t primary;
    uint64_t shadow;
    uint64_t secondary;
} rg_ray_counts;

typedef struct rg_stats {
    rg_ray_counts rays;
    float kernel_ms;           /* HIP-event time of the render launch(es) on the render stream */
    int32_t error_pixel;       /* first pixel (linear index) that raised a device error, or -1 */
    uint32_t _pad;
} rg_stats;

/* Row selection for sharded renders: the frame is cut into tiles of
 * `tile_rows` rows; this call renders tiles t with t % tile_stride == tile_offset,
 * packed densely into the output in increasing t (the last tile may be partial
 * and is zero-padded in the output to a full tile).  {tile_rows=height,
 * tile_stride=1, tile_offset=0} is the whole frame.  */
typedef struct rg_tiling {
    uint32_t tile_rows;
    uint32_t tile_stride;
    uint32_t tile_offset;
} rg_tiling;

typedef struct rg_scene rg_scene;   /* opaque device-resident scene */

/* ---------------------------------------------------------------- API */

int32_t rg_abi_version(void);
const char *rg_status_string(int32_t status);

/* Number of HIP devices visible (0 if none / runtime missing). */
int32_t rg_device_count(void);

/* Copy the scene to `device` (SoA body tables, material/light tables, RGBA8
 * textures).  The caller keeps ownership of `desc` and its arrays.
 * Replaces Scene's deserialised in-memory form (scene.rs:11-19). */
rg_status rg_scene_create(const rg_scene_desc *desc, int32_t device, rg_scene **out);
void rg_scene_destroy(rg_scene *scene);

/* Override the recursion cap of an uploaded scene (main.rs:119-123 clamps it;
 * the depth-5 configs set it directly, scene.rs:16 is a pub field). */
rg_status rg_scene_set_max_depth(rg_scene *scene, uint32_t max_recursion_depth);

/* A movable camera: the eye point and the basis the primary rays are built on.  For pixel (x, y)
 * of a width x height frame, with sx, sy the reference's sensor coordinates (ray.rs:43-51):
 *   D.k = (right.k * sx + up.k * sy) + forward.k     (k = x, y, z; f64, in this order, unfused)
 *   ray = Ray::new(eye, normalize(D))                a primary ray at depth 0
 * Every member finite, forward not all zero; the basis need be neither unit nor orthogonal.
 * {eye 0, right (1,0,0), up (0,1,0), forward (0,0,-1)} is the reference's Ray::create_prime
 * (ray.rs:37-54) bit for bit. */
typedef struct rg_camera {
    double eye[3], right[3], up[3], forward[3];
} rg_camera;

/* forward = normalize(target - eye), right = normalize(cross(forward, up)), up = cross(right,
 * forward).  Pure host code.  RG_ERR_INVALID_ARGUMENT for a null pointer, target == eye, a
 * non-finite input, cross(forward, up) == 0 or a result that is no camera. */
rg_status rg_camera_look_at(const double eye[3], const double target[3], const double up[3], rg_camera *out);

/* The camera of every later render of `scene` that goes through the tiled launch: rg_render_image,
 * rg_render_tiles / _async / _pipelined, rg_render_stream, rg_render_image_aa / rg_render_aa_async,
 * rg_render_image_aa_adaptive / rg_render_aa_adaptive, rg_render_multi (both modes; its replicas
 * follow) and rg_frames_*, and of rg_render_aov / rg_render_aov_async.  rg_trace is unaffected; error codes and error_pixel keep their meaning.
 * NULL restores the reference's view, and with it exactly the kernels the scene launched before.
 * The camera is host state: it is read when a launch is enqueued and travels by value in the
 * kernel's arguments, so changing it between launches on different streams needs no
 * synchronisation and launches in flight keep theirs.  RG_ERR_INVALID_ARGUMENT for a non-finite
 * member or a zero forward (the scene keeps the camera it had). */
rg_status rg_scene_set_camera(rg_scene *scene, const rg_camera *camera);

/* Blocking whole-frame render into a caller-owned host buffer of
 * width*height*4 bytes (row-major RGBA8, alpha 255).
 * Replaces rendering::render_image (rendering.rs:24-38). `stats` may be NULL.
 * Into a pinned `rgba_out` (rg_host_register, or memory from hipHostMalloc)
 * a heavy (trace-dominated) scene renders in ONE launch whose pixel stores go
 * over PCIe straight into the buffer; otherwise the frame renders in row
 * bands whose device-to-host copies overlap the later bands' renders (the DMA
 * lands directly in a pinned buffer; a pageable one is filled from pinned
 * staging by several host threads).  Any max_recursion_depth renders (scene.rs:16 is a u32): depths
 * above 65 keep their shading frames in device memory, 88 B per open frame
 * per thread of a persistent grid; when that exceeds half the free device
 * memory (capped at 16 GiB) the grid shrinks to fit -- slower, same frame --
 * and only when a single block's frames do not fit does the call return
 * RG_ERR_OUT_OF_MEMORY (depth ~ 10^6 and up).  On a device error
 * (RG_ERR_AABB_NORMAL / _NAN_DISTANCE / _TRANSMISSION: the reference's
 * panics) the frame is still delivered and stats->error_pixel names the first
 * (lowest-index) pixel that raised it. */
rg_status rg_render_image(const rg_scene *scene, uint32_t width, uint32_t height,
                          uint8_t *rgba_out, rg_stats *stats);

/* rg_render_image with samples x samples rays per pixel on a regular sub-pixel grid,
 * box-filtered (supersampled anti-aliasing; samples 1..8).  The rays are those of the
 * samples*width x samples*height frame (ray.rs:43-49 puts them exactly on the sub-pixel
 * grid).  Per pixel and channel, in f32: every sample s is clamped (s if 0 <= s <= 1, 1 if
 * s > 1, else 0: negatives and NaN), the clamped samples are added one by one to 0, sample
 * rows outer, columns inner, the sum is divided by samples*samples, and the byte is
 * `(mean * 255.0) as u8` (color.rs:32-37) with alpha 255.  `rgb_out` (nullable, host,
 * width*height*3 floats) receives the means.  samples == 1 gives the bytes of
 * rg_render_image.  `stats` counts the rays of every sample; on a device error the frame
 * is still delivered, the status is the reference's panic code and stats->error_pixel is
 * the output pixel that contains the lowest-index failing sample.  RG_ERR_INVALID_ARGUMENT
 * for null pointers, zero sizes, samples outside 1..8 or a sample frame of 2^32 pixels or
 * more; RG_ERR_PORTRAIT for width < height. */
rg_status rg_render_image_aa(const rg_scene *scene, uint32_t width, uint32_t height, uint32_t samples,
                             uint8_t *rgba_out, float *rgb_out, rg_stats *stats);

/* Device-resident rg_render_image_aa: `rgba_dev` (width*height*4 bytes) and `rgb_dev`
 * (nullable, width*height*3 floats) are device pointers on the scene's device.  The work is
 * ordered after everything enqueued on `stream` (a hipStream_t; NULL = null stream) so far,
 * and later work on `stream` is ordered after it; in between it runs on two streams of the
 * scene's own.  Asynchronous unless `stats` is non-NULL, in which case the call
 * synchronises `stream` and fills ray counts, time and errors (as rg_render_tiles_async).
 * Without `stats` device errors are not reported (rg_stream_status does not see this
 * call's launches).  Calls on one scene must come from one host thread at a time. */
rg_status rg_render_aa_async(const rg_scene *scene, uint32_t width, uint32_t height, uint32_t samples,
                             uint8_t *rgba_dev, float *rgb_dev, void *stream, rg_stats *stats);

/* The resolve of rg_render_image_aa alone, on `device`, host buffers: `rgb_in` is
 * (samples*height) x (samples*width) x 3 floats, row-major; `rgba_out` width*height*4
 * bytes; `rgb_out` nullable, width*height*3 floats.  Blocking. */
rg_status rg_resolve_box(int32_t device, const float *rgb_in, uint32_t width, uint32_t height,
                         uint32_t samples, uint8_t *rgba_out, float *rgb_out);

/* Adaptive anti-aliasing: rg_render_image_aa that traces the samples x samples rays only of
 * pixels on edges of the 1-sample frame.  With `base` the frame of rg_render_image:
 *   contrast  m(p) = max |base[p][c] - base[q][c]| as integers, over c in {R, G, B} and the up
 *             to eight neighbours q of p inside the frame (0 without neighbours; alpha ignored)
 *   mask      flag(p) = m(p) >= threshold (0..256: 0 flags every pixel, 256 none)
 *   pixel     flagged: the box resolve of its samples x samples samples, exactly as
 *             rg_render_image_aa; unflagged: the base pixel's bytes, and for `rgb_out` its f32
 *             RGB clamped as a sample (the samples = 1 resolve)
 * `mask_out` (nullable, host, width*height bytes) receives the mask, 1 = supersampled.  Rays
 * (`stats`): for threshold >= 1 and samples >= 2 those of the base frame plus those of exactly
 * the samples*samples samples of every flagged pixel (primary == width*height +
 * samples*samples*flagged); threshold 0 is rg_render_image_aa (no base pass), samples 1 is
 * rg_render_image (the mask is still produced).  On a device error the frame is still
 * delivered and stats->error_pixel is the lower of the base pass's failing pixel and the output
 * pixel that contains the lowest-index failing traced sample, the status that pixel's (a tie:
 * the base pass's).  Arguments as rg_render_image_aa, and RG_ERR_INVALID_ARGUMENT for
 * threshold > 256.  raingun_amd/aa.py restates the result in numpy (resolve_adaptive). */
rg_status rg_render_image_aa_adaptive(const rg_scene *scene, uint32_t width, uint32_t height,
                                      uint32_t samples, uint32_t threshold, uint8_t *rgba_out,
                                      float *rgb_out, uint8_t *mask_out, rg_stats *stats);

/* Device-resident rg_render_image_aa_adaptive: `rgba_dev`, `rgb_dev` (nullable) and `mask_dev`
 * (nullable) are device pointers on the scene's device.  The work is ordered after everything
 * enqueued on `stream` so far and later work on `stream` after it.  BLOCKING: the host reads
 * the per-band tile counts between the 1-sample pass and the sample launches, and the call
 * returns with `stream` idle.  `stats` nullable. */
rg_status rg_render_aa_adaptive(const rg_scene *scene, uint32_t width, uint32_t height,
                                uint32_t samples, uint32_t threshold, uint8_t *rgba_dev,
                                float *rgb_dev, uint8_t *mask_dev, void *stream, rg_stats *stats);

/* The edge detector of rg_render_image_aa_adaptive alone, on `device`, host buffers, blocking
 * (as rg_resolve_box): `rgba_in` width*height packed RGBA8 pixels (any shape: portrait too),
 * `mask_out` width*height bytes, *flagged (nullable) the number of ones.
 * RG_ERR_INVALID_ARGUMENT for null buffers, zero sizes, threshold > 256 or 2^32 pixels or more. */
rg_status rg_edge_mask(int32_t device, const uint8_t *rgba_in, uint32_t width, uint32_t height,
                       uint32_t threshold, uint8_t *mask_out, uint32_t *flagged);

/* Page-lock a caller buffer (hipHostRegister) so rg_render_image / rg_render_tiles
 * / rg_render_multi DMA straight into it; unregister before freeing it.  Optional:
 * pageable buffers work too (staged).  A Rust caller registers its
 * ImageBuffer's Vec once and reuses it across frames. */
rg_status rg_host_register(void *ptr, size_t bytes);
rg_status rg_host_unregister(void *ptr);

/* Device-resident variant used by sharded / benchmark callers: renders the
 * tiles selected by `tiling` into `rgba_dev` (device pointer on the scene's
 * device, tiles_selected*tile_rows*width*4 bytes), on HIP stream `stream`
 * (a hipStream_t; NULL = null stream).  `rgb_dev` (nullable, device) receives
 * the pre-quantisation f32 RGB (3 floats per pixel, same packing) for float
 * parity checks.  Asynchronous unless `stats` is non-NULL, in which case the
 * call synchronises `stream` and fills ray counts, kernel time and errors.
 * Launches of one scene on DISTINCT streams may be in flight together (frames
 * in flight): each stream has its own launch state (ray counters, tile queue,
 * error word), created on the stream's first use.  Calls on one scene must
 * come from one host thread at a time.  The launch is sized for its own
 * latency (the whole GPU for this one frame). */
rg_status rg_render_tiles_async(const rg_scene *scene, uint32_t width, uint32_t height,
                                const rg_tiling *tiling, uint8_t *rgba_dev, float *rgb_dev,
                                void *stream, rg_stats *stats);

/* rg_render_tiles_async for a caller that keeps several frames in flight on
 * distinct streams (rg_frames, bench.py): asynchronous, and trace-heavy scenes
 * size their persistent grid for throughput -- a small launch takes a third
 * of the GPU or more with at least 32 tiles per wave, and the other frames in
 * flight fill the rest -- rather than for one launch's latency.  Same output. */
rg_status rg_render_tiles_pipelined(const rg_scene *scene, uint32_t width, uint32_t height,
                                    const rg_tiling *tiling, uint8_t *rgba_dev, float *rgb_dev,
                                    void *stream);

/* Forget the launch state of `stream` (before the caller destroys that stream);
 * the null stream's state lives as long as the scene. */
rg_status rg_scene_release_stream(rg_scene *scene, void *stream);

/* Status of the launches enqueued on `stream` since the previous call:
 * synchronises the stream, returns the first (lowest-pixel) device error any
 * of them raised (RG_OK if none) with its pixel in *error_pixel (nullable;
 * -1 if none), and clears it.  For asynchronous callers (stats == NULL),
 * whose launches otherwise report nothing. */
rg_status rg_stream_status(const rg_scene *scene, void *stream, int32_t *error_pixel);

/* Host-buffer variant of rg_render_tiles_async (blocking).  rgb_out nullable. */
rg_status rg_render_tiles(const rg_scene *scene, uint32_t width, uint32_t height,
                          const rg_tiling *tiling, uint8_t *rgba_out, float *rgb_out,
                          rg_stats *stats);

/* Number of output rows a tiling produces for `height` (tiles selected * tile_rows). */
uint32_t rg_tiling_rows(uint32_t height, const rg_tiling *tiling);

/* Tile-completion streaming (replaces render_image_stream, rendering.rs:40-69,
 * which sends one RenderedPixel per pixel over an mpsc channel): ONE launch
 * renders the frame into page-locked host memory and publishes every finished
 * tile; `on_tile` receives each band of `tile_rows` rows, in row order, as soon
 * as the band is complete, while the kernel renders on.  A non-zero return
 * from `on_tile` cancels: the kernel takes no further tiles (the reference's
 * `.all` stops when the channel closes) and the call returns RG_ERR_CANCELLED.
 * The band pointer is valid only during the callback. */
typedef int32_t (*rg_tile_callback)(uint32_t row_begin, uint32_t rows, uint32_t width,
                                    const uint8_t *rgba, void *user);
rg_status rg_render_stream(const rg_scene *scene, uint32_t width, uint32_t height,
                           uint32_t tile_rows, rg_tile_callback on_tile, void *user,
                           rg_stats *stats);

/* Closest-hit query over all bodies (Scene::trace, scene.rs:34-39) for n rays
 * given as {origin.xyz, direction.xyz} doubles (host buffers).  dist[i] is the
 * hit distance and body[i] the body index, or body[i] = -1 on a miss. */
rg_status rg_trace(const rg_scene *scene, const double *rays, uint32_t n,
                   double *dist, int32_t *body);

/* AOV layers (auxiliary output variables, a G-buffer): what lies under each pixel.  The ray of pixel
 * (x, y) is exactly the ray rg_render_image traces for it: Ray::create_prime (ray.rs:37-54), or the
 * ray of rg_scene_set_camera.  One ray per pixel, at depth 0, whatever the scene's max depth:
 * rays.primary == the pixels rendered, shadow and secondary are 0.  Layers are row-major. */
typedef struct rg_aov {          /* every member nullable; at least one non-null */
    int32_t *body;               /* YAML index of the primary hit, -1 on a miss                      */
    double  *depth;              /* its Scene::trace distance t (scene.rs:34-39), +inf on a miss      */
    float   *normal;             /* 3 per pixel: (f32) of each f64 component of surface_normal(body, hit),
                                    hit = origin + direction * t (rendering.rs get_color); the reference's
                                    geometric normal, never flipped; 0,0,0 on a miss                   */
    float   *uv;                 /* 2 per pixel: texture_coords(body, hit) before the material's offsets;
                                    0,0 on a miss and for AABBs                                        */
    float   *albedo;             /* 3 per pixel: Material::color at the hit (texture texel or flat colour,
                                    material.rs:62-68); the scene's default_color on a miss            */
} rg_aov;

/* Blocking whole-frame AOV render into host buffers (pageable or pinned) of width*height elements
 * per requested layer.  The frame is delivered on every device error: RG_ERR_NAN_DISTANCE where
 * rg_trace raises it; RG_ERR_AABB_NORMAL when `normal` is requested and surface_normal finds no face
 * (bodies.rs:324; that pixel's normal is 1,0,0 as in get_color); stats->error_pixel is the lowest
 * failing pixel.  RG_ERR_PORTRAIT for width < height; RG_ERR_INVALID_ARGUMENT for a null scene or
 * `out`, all five pointers null, zero sizes or 2^32 pixels or more.  `stats` may be NULL. */
rg_status rg_render_aov(const rg_scene *scene, uint32_t width, uint32_t height,
                        const rg_aov *out /* host */, rg_stats *stats);

/* Device-resident rg_render_aov of the tiles selected by `tiling`, with rg_render_tiles_async's packing
 * and stream contract: `dev` holds device pointers on the scene's device (rg_tiling_rows x width
 * elements per requested layer); each stream has its own launch context, launches of one scene on
 * distinct streams may be in flight together, the camera is read at enqueue and travels by value, and
 * the call is asynchronous unless `stats` is non-NULL (then it synchronises `stream`; without it
 * rg_stream_status reports device errors).  Padding rows of a partial last tile hold body -1, depth
 * +inf and zeros in the other layers.  Also RG_ERR_INVALID_ARGUMENT for a null or bad tiling. */
rg_status rg_render_aov_async(const rg_scene *scene, uint32_t width, uint32_t height,
                              const rg_tiling *tiling, const rg_aov *dev /* device */,
                              void *stream, rg_stats *stats);

/* Single-process multi-GPU render (SURVEY.md §8(b),(e)): the same frame as
 * rg_render_image, split over `ngpus` devices -- the scene's device first,
 * then the next visible devices in order -- in `tile_rows`-row tiles dealt
 * round-robin (tile t -> device t % ngpus; 0 = 8 rows).  Each device renders
 * its tiles with its own replica of the scene (made on first use and kept)
 * in row bands, and after each band copies that band's tiles straight to
 * their image rows of `rgba_out` (width*height*4 bytes, host) with one
 * strided copy over its OWN PCIe link, overlapped with its later bands: N
 * links carry 1/N of the frame each (a pageable buffer is fed from a pinned
 * frame by host threads).  The RCCL path -- one ncclGather over xGMI to the
 * scene's device, re-interleave, one copy -- remains available through
 * rg_debug_set_multi (mode 1); its communicators come from ncclCommInitAll in
 * this process (RCCL loaded at run time: the librccl already in the process,
 * else $RG_RCCL_LIBRARY, else librccl.so.1; RG_ERR_COLLECTIVE if it cannot be
 * loaded).  No torch, no launcher: the drop-in for the reference's one
 * blocking call (rendering.rs:24-38, src/render.rs:55) on a whole node.
 * `stats` sums the devices' rays; on device errors error_pixel is the lowest
 * failing pixel of any device; kernel_ms is device 0's render span (its
 * launches, not the other devices' work or the copies to the host).  Every
 * copy into rgba_out has landed when the call returns, on errors too. */
rg_status rg_render_multi(const rg_scene *scene, uint32_t width, uint32_t height, int32_t ngpus,
                          uint32_t tile_rows, uint8_t *rgba_out, rg_stats *stats);

/* A thin lens: depth of field for the supersampled frames.  aperture: the lens radius in world units;
 * focus: the distance of the plane in focus along the camera's forward, in units of |forward|.
 * It applies to the samples x samples rays per pixel of rg_render_image_aa and rg_render_aa_async for
 * samples >= 2, and to nothing else: with samples == 1, without a lens or with aperture == 0 those two
 * calls launch the kernels and give the bytes they give today.  Deterministic, no random numbers: with
 * (E, R, U, F) the scene's camera (or {0, (1,0,0), (0,1,0), (0,0,-1)} without one), k = samples and sx, sy
 * the sensor coordinates of pixel (X, Y) of the kW x kH sample frame -- f64, unfused, in this order:
 *   D.c = (R.c * sx + U.c * sy) + F.c
 *   s = (Y % k) * k + (X % k);  (pu, pv) = points_k[s]           the sample's point of the unit disk
 *   n = (Y / k) * W + (X / k);  h = lowbias32(n)                 the output pixel's hash (u32):
 *         n ^= n >> 16; n *= 0x7feb352d; n ^= n >> 15; n *= 0x846ca68b; n ^= n >> 16
 *   (c, g) = rotations[h & 63]                                   that pixel's turn of the lens disk
 *   qu = c * pu - g * pv;  qv = g * pu + c * pv
 *   O.c = LR.c * qu + LU.c * qv           LR = normalize(R) * aperture, LU = normalize(U) * aperture
 *   ray = Ray::new(E + O, normalize(D * focus - O))              a primary ray at depth 0
 * points_k and rotations are rg_lens_tables'.  Every sample of a pixel meets the plane in focus where the
 * pinhole ray of its sub-pixel does; the per-pixel turn keeps an out-of-focus object from showing as k^2
 * ghost copies. */
typedef struct rg_lens { double aperture, focus; } rg_lens;

/* The lens of every later rg_render_image_aa / rg_render_aa_async of `scene`; NULL or aperture == 0: the
 * pinhole again, and with it exactly the kernels those calls launched before.  Host state like the camera:
 * read when a launch is enqueued, carried by value in the kernel's arguments (launches in flight keep
 * theirs; the tables on the device are made once per scene and never rewritten), and followed by
 * rg_render_multi's replicas.  The entry points that trace one ray per pixel ignore it: rg_render_image,
 * rg_render_tiles / _async / _pipelined, rg_render_stream, rg_render_multi, rg_frames_*, rg_render_aov /
 * _async and rg_trace.  While a lens with aperture > 0 is set, rg_render_image_aa_adaptive and
 * rg_render_aa_adaptive return RG_ERR_INVALID_ARGUMENT: their edge mask comes from a pinhole frame and
 * says nothing about defocus.  Ray counts, error_pixel and status codes of the two AA calls keep their
 * meaning; while the scene's camera has a zero right or up (no axis to span the lens disk with) they
 * return RG_ERR_INVALID_ARGUMENT for samples >= 2.  RG_ERR_INVALID_ARGUMENT for a null scene, a non-finite
 * member, aperture < 0 or focus <= 0 (the scene keeps the lens it had). */
rg_status rg_scene_set_lens(rg_scene *scene, const rg_lens *lens);

/* The lens's two tables, pure host code.  points: 2 * samples^2 doubles, the concentric (Shirley-Chiu) map
 * onto the unit disk of the cell centres ((i + 0.5) / samples, (j + 0.5) / samples) at index j * samples + i
 * (samples == 1 and the centre cell of an odd samples: exactly (0, 0)).  rotations (nullable): 128 doubles,
 * (cos, sin) of 2 pi m / 64 for m = 0 .. 63.  RG_ERR_INVALID_ARGUMENT for samples outside 1 .. 8 or a null
 * `points`. */
rg_status rg_lens_tables(uint32_t samples, double *points, double *rotations);

/* Area lights: soft shadows for the supersampled frames.  A spherical light l gets a radius radii[l] >= 0
 * in world units; a directional light has no position and stays hard: its radius must be 0.
 * The radii apply to the samples x samples rays per pixel of rg_render_image_aa and rg_render_aa_async for
 * samples >= 2, and to nothing else: with samples == 1, or with every radius 0, those two calls launch the
 * kernels and give the bytes they give today.  Deterministic, no random numbers: with k = samples, (X, Y) a
 * pixel of the kW x kH sample frame (Y the row of the whole frame), l the light's index in the scene's
 * order and v its position -- u32 wrap-around, then f64, unfused, in this order:
 *   s = (Y % k) * k + (X % k)                          the sample
 *   n = (Y / k) * W + (X / k)                          the output pixel
 *   g = lowbias32(n ^ ((l + 1) * 0x9e3779b9))          the hash of rg_lens above
 *   j = (s + (g >> 6)) % (k * k)                       this pixel's and light's shift through the points
 *   (c, e) = rotations[g & 63]                         rg_lens_tables' 64 turns, here about world z
 *   (px, py, pz) = sphere_points_k[j]                  rg_area_tables'
 *   qx = c * px - e * py;  qy = e * px + c * py;  qz = pz
 *   position.c = v.c + radii[l] * q.c                  for every spherical light, radius 0 included
 * Everything the reference does with the light's position (lights.rs:36-58: direction_from, distance, the
 * intensity's falloff) uses `position` instead, for every hit of that sample's whole ray tree: primary,
 * reflected and transmitted hits alike.  The samples of a pixel see k^2 points spread evenly over the
 * light's sphere, so a shadow's edge resolves into a penumbra.  Area lights combine with the camera and
 * with the lens.
 *
 * rg_scene_set_light_radii sets the radii of every later rg_render_image_aa / rg_render_aa_async of `scene`;
 * NULL: point lights again, and with them (as with every radius 0) exactly the kernels those calls launched
 * before.  n must be the scene's light count.  Unlike the camera and the lens the radii are one per light
 * and live in a table on the device, which launches read by reference: the call BLOCKS until the scene's
 * device is idle before it rewrites that table, and launches enqueued later see the new radii.
 * rg_render_multi's replicas copy the radii.  The entry points that trace one ray per pixel ignore them:
 * rg_render_image, rg_render_tiles / _async / _pipelined, rg_render_stream, rg_render_multi, rg_frames_*,
 * rg_render_aov / _async and rg_trace.  While any radius is > 0, rg_render_image_aa_adaptive and
 * rg_render_aa_adaptive return RG_ERR_INVALID_ARGUMENT: their edge mask comes from a hard-shadow frame and
 * says nothing about penumbrae.  Ray counts, error_pixel and status codes of the two AA calls keep their
 * meaning.  RG_ERR_INVALID_ARGUMENT for a null scene, n other than the light count, a non-finite or
 * negative radius, or a non-zero radius on a directional light (the scene keeps the radii it had). */
rg_status rg_scene_set_light_radii(rg_scene *scene, const double *radii, uint32_t n);

/* The area lights' points, pure host code.  points: 3 * samples^2 doubles, uniform on the unit sphere: cell
 * (i, j) of the samples x samples grid, at index j * samples + i, with u = (i + 0.5) / samples,
 * v = (j + 0.5) / samples:  z = 1 - 2u, rho = sqrt(1 - z z), phi = 2 pi v, point = (rho cos phi, rho sin phi, z).
 * RG_ERR_INVALID_ARGUMENT for samples outside 1 .. 8 or a null `points`. */
rg_status rg_area_tables(uint32_t samples, double *points);

/* Ambient occlusion: per pixel, the share of the hemisphere above the primary hit that is open.  The companion
 * of the AOV layers: samples x samples any-hit rays per hit pixel, no lights, no shading.  Deterministic, no
 * random numbers; everything f64, unfused, in the order written.  For pixel (x, y) of the frame:
 *   1. the primary ray (o, d) is the ray rg_render_aov traces for that pixel (create_prime, or the ray of
 *      rg_scene_set_camera), closest hit by Scene::trace (scene.rs:34-39).  On a miss ao = 1.0f and no further
 *      ray is traced.  RG_ERR_NAN_DISTANCE where rg_render_aov raises it.
 *   2. h = o + d * t;  n = surface_normal(body, h) -- without an AABB face (1,0,0) and RG_ERR_AABB_NORMAL, as
 *      get_color does.
 *   3. m = normalize(n) (plane and disk normals are the YAML's, not unit);  nf = m if dot(m, d) <= 0, else -m:
 *      the side the ray came from.
 *   4. O.c = h.c + nf.c * bias
 *   5. s = copysign(1.0, nf.z);  a = -1.0 / (s + nf.z);  b = (nf.x * nf.y) * a         (Duff et al.)
 *      T = (1.0 + (s * nf.x) * (nf.x * a),  s * b,  (-s) * nf.x)
 *      B = (b,  s + (nf.y * nf.y) * a,  -nf.y)
 *   6. p = y * width + x (y the row of the whole frame);  hsh = lowbias32(p), the hash of rg_lens;
 *      (c, g) = rotations[hsh & 63], rg_lens_tables' 64 turns;
 *      Tr.c = c * T.c + g * B.c;  Br.c = c * B.c - g * T.c               once per pixel
 *   7. for sample j = 0 .. k^2 - 1, in this order:  (px, py, pz) = ao_points_k[j], rg_ao_tables';
 *      D.c = (Tr.c * px + Br.c * py) + nf.c * pz;  ray = Ray::new(O, normalize(D)).
 *      The ray is occluded iff Scene::trace finds a hit with !(t > radius): the rule of rendering.rs:150-155 with
 *      `radius` in place of the light's distance, the scene.rs:38 panic (RG_ERR_NAN_DISTANCE) included where two
 *      hits are compared and one is NaN.
 *   8. ao = (float)open / (float)(k * k), open the number of rays not occluded.
 * Ray counts: primary == the pixels rendered, shadow == k^2 x the hit pixels (AO rays count in the shadow class),
 * secondary == 0.  Ignored by design: the scene's lens, its light radii, its lights and max_recursion_depth.
 * rg_render_multi and rg_frames_* have no AO mode. */
typedef struct rg_ao {
    uint32_t samples;   /* k: k x k rays per hit pixel, 1..8 */
    uint32_t _pad;
    double radius;      /* > 0, may be +inf: a ray is occluded by a hit at distance t with !(t > radius) */
    double bias;        /* >= 0, finite: the origin's offset along the facing normal (the reference's own is 1e-13) */
} rg_ao;

/* The AO pass's points, pure host code.  points: 3 * samples^2 doubles; the point at index j * samples + i is
 * (pu, pv, sqrt(fmax(0.0, (1.0 - pu*pu) - pv*pv))) with (pu, pv) rg_lens_tables' point of that index: the unit
 * disk lifted onto the hemisphere, so the rays are cosine-weighted (Malley).  samples == 1 and the centre cell of
 * an odd samples: exactly (0, 0, 1).  The device holds the points of samples = 1 .. 8 in a table made once per
 * scene on the first AO frame and never rewritten.  RG_ERR_INVALID_ARGUMENT for samples outside 1 .. 8 or a null
 * `points`. */
rg_status rg_ao_tables(uint32_t samples, double *points);

/* Blocking whole-frame AO render into a host buffer (pageable or pinned) of width*height floats, row-major.  The
 * frame is delivered on the reference's panics (RG_ERR_NAN_DISTANCE, RG_ERR_AABB_NORMAL); stats->error_pixel is
 * the lowest failing pixel.  Status codes as rg_render_aov's, plus RG_ERR_INVALID_ARGUMENT for a null `ao` or
 * `ao_out`, samples outside 1 .. 8, radius NaN or <= 0, bias negative or not finite.  A rejected call writes
 * nothing.  `stats` may be NULL. */
rg_status rg_render_ao(const rg_scene *scene, uint32_t width, uint32_t height, const rg_ao *ao,
                       float *ao_out /* host, width*height */, rg_stats *stats);

/* Device-resident rg_render_ao of the tiles selected by `tiling`, with rg_render_aov_async's tiling, packing and
 * stream contract: `ao_dev` is device memory on the scene's device (rg_tiling_rows x width floats); each stream
 * has its own launch context, launches of one scene on distinct streams may be in flight together, the camera is
 * read at enqueue and travels by value as `ao` does, and the call is asynchronous unless `stats` is non-NULL (then
 * it synchronises `stream`; without it rg_stream_status reports device errors).  Padding rows of a partial last
 * tile hold 0.0f.  Also RG_ERR_INVALID_ARGUMENT for a null or bad tiling. */
rg_status rg_render_ao_async(const rg_scene *scene, uint32_t width, uint32_t height, const rg_tiling *tiling,
                             const rg_ao *ao, float *ao_dev /* device, rg_tiling_rows x width */, void *stream,
                             rg_stats *stats);

/* The edge-stopping filter of the AO pass: a tent over (2r+1) x (2r+1) pixels that takes in only neighbours on the
 * same body whose normal agrees with the centre's.  The AO pass dithers by design (an integer count over k^2, turned
 * per pixel); this is the geometry-aware filter that finishes it.  Its guides are the layers exactly as
 * rg_render_aov delivers them (plane and disk normals are not unit).  No depth guide: all four body kinds are
 * convex, so body and normal separate everything depth would.  Everything f32, unfused, in the order written.  Per
 * pixel, row-major: `ao` (f32), `body` (i32, -1 on a miss), `normal` (3 x f32).  For pixel p = (x, y), b = body[p]:
 *   b < 0:  out[p] = ao[p], bits unchanged.
 *   else    nn_p = (n_p.x*n_p.x + n_p.y*n_p.y) + n_p.z*n_p.z;  t = normal_min * normal_min
 *           sum = 0.0f;  wsum = 0 (an integer)
 *           for dy = -r .. r (outer), dx = -r .. r (inner), q = (x + dx, y + dy); q outside the frame is skipped:
 *               w = (r + 1 - |dx|) * (r + 1 - |dy|)                       a tent, an integer <= 81
 *               d = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z
 *               q is accepted iff it is the centre, or body[q] == b && d > 0.0f && d*d >= t * (nn_p * nn_q),
 *               nn_q as nn_p; a NaN compares false
 *               accepted:  sum = sum + (float)w * ao[q];  wsum += w
 *           out[p] = sum / (float)wsum                                    wsum <= 6561; the centre makes it >= (r+1)^2
 * The sum's order is part of the contract: the result is the same bits on every device and in
 * raingun_amd/ambient.py's numpy restatement (filter_ao). */
typedef struct rg_ao_filter_desc {
    uint32_t radius;     /* r: 1..8 */
    float normal_min;    /* in [0, 1]: the least cosine between the centre's normal and an accepted neighbour's */
} rg_ao_filter_desc;

/* The filter alone, on `device`, host buffers, blocking (as rg_resolve_box / rg_edge_mask): any shape, portrait
 * too.  `ao_out` (width*height floats) may not alias `ao_in`.  RG_ERR_INVALID_ARGUMENT for null buffers, a null
 * `filter`, zero sizes, 2^32 pixels or more, radius outside 1..8, normal_min NaN or outside [0, 1], or aliasing
 * buffers, or a buffer that is not 4-byte aligned.  A rejected call writes nothing. */
rg_status rg_ao_filter(int32_t device, const float *ao_in, const int32_t *body, const float *normal,
                       uint32_t width, uint32_t height, const rg_ao_filter_desc *filter, float *ao_out);

/* rg_ao_filter on device memory of `device` (4-byte aligned; nothing more is asked), enqueued on `stream` (a hipStream_t; NULL = null
 * stream); asynchronous.  Same rejections. */
rg_status rg_ao_filter_async(int32_t device, const float *ao_dev, const int32_t *body_dev, const float *normal_dev,
                             uint32_t width, uint32_t height, const rg_ao_filter_desc *filter, float *ao_out_dev,
                             void *stream);

/* An ambient term: the filtered AO pass multiplied into an ambient light and added to the supersampled beauty frame.
 * The reference has no ambient light, so what no light reaches renders black there; this is an addition, and colour
 * (0, 0, 0) gives the bytes of rg_render_image_aa at the same `samples`.
 *   share[b]  one f32 per body, from the scene description: diffuse: albedo; reflecting: (1.0f - reflectivity) *
 *             albedo; refractive: 0.0f -- the weight get_color gives shade_diffuse (rendering.rs:86-118) times the
 *             albedo of light_reflected (rendering.rs:165).  The AO pass is cosine-weighted, so the / pi of
 *             light_reflected and the hemisphere's pi cancel: `color` means "this radiance from every open direction".
 *   compose   per pixel p and channel c, f32, unfused:
 *               hit (b = body[p] >= 0):  v = rgb[p].c + (color.c * albedo[p].c) * (share[b] * aof[p])
 *               miss:                    v = rgb[p].c
 *             then v clamped as a sample (v if 0 <= v <= 1, 1 if v > 1, else 0) and the byte `(v * 255.0) as u8`,
 *             alpha 255: the rule of rg_render_image_aa's resolve.
 *   rgb       the clamped f32 means of rg_render_aa_async at `samples`;  albedo, body: rg_render_aov's layers;
 *   aof       rg_ao_filter{filter_radius, normal_min} of rg_render_ao{ao} guided by rg_render_aov's body and normal,
 *             or the raw pass when filter_radius is 0.
 * The camera, the lens and the light radii are honoured because the passes honour them (the AOV and AO passes trace
 * the pinhole ray of the pixel's centre).  There is no adaptive variant, and rg_render_multi and rg_frames_* have no
 * ambient mode. */
typedef struct rg_ambient {
    float color[3];          /* finite, >= 0 */
    uint32_t samples;        /* the beauty frame's samples per pixel side, 1..8 */
    rg_ao ao;
    uint32_t filter_radius;  /* 0..8; 0: unfiltered */
    float normal_min;        /* in [0, 1] */
} rg_ambient;

/* Blocking whole frame with an ambient term into host buffers: `rgba_out` width*height*4 bytes; `rgb_out` (nullable)
 * width*height*3 floats, the clamped v; `ao_out` (nullable) width*height floats, aof.  On the scene's device it runs,
 * in order, the supersampled beauty frame, the AOV pass (body, normal, albedo), the AO pass, the filter and the
 * compose, then copies out.  `stats` (nullable) is the sum of the three tracing passes: primary == pixels x
 * (samples^2 + 2), shadow == the beauty frame's + k^2 x hit pixels, secondary == the beauty frame's; kernel_ms adds the
 * three passes' and the two image kernels'.  On a device error (the reference's panics) the frame is still delivered,
 * error_pixel is the lowest failing pixel over the three passes and the status that pixel's; a tie goes to the beauty
 * frame, then the AOV pass, then the AO pass.  RG_ERR_PORTRAIT for width < height; RG_ERR_INVALID_ARGUMENT for null
 * `scene`, `ambient` or `rgba_out`, zero sizes, a sample frame of 2^32 pixels or more, a colour that is negative or
 * not finite, samples outside 1..8, an `ao` rg_render_ao rejects, filter_radius above 8, normal_min NaN or outside
 * [0, 1].  A rejected call writes nothing. */
rg_status rg_render_image_ambient(const rg_scene *scene, uint32_t width, uint32_t height, const rg_ambient *ambient,
                                  uint8_t *rgba_out, float *rgb_out, float *ao_out, rg_stats *stats);

/* Device-resident rg_render_image_ambient: `rgba_dev`, `rgb_dev` (nullable) and `ao_dev` (nullable) are device
 * pointers on the scene's device, each 4-byte aligned (`rgba_dev` too: the compose stores whole pixels;
 * RG_ERR_INVALID_ARGUMENT otherwise).  The work is ordered after everything enqueued on `stream` so far and later work on
 * `stream` after it (the beauty frame runs as rg_render_aa_async does); the layers between the passes live in
 * scratch the scene keeps per stream, so frames on distinct streams may be in flight together.  Asynchronous unless
 * `stats` is non-NULL: then every tracing pass synchronises `stream`.  Without `stats` the beauty frame's device
 * errors are not reported (rg_stream_status sees the AOV and AO passes).  Calls on one scene must come from one host
 * thread at a time. */
rg_status rg_render_ambient_async(const rg_scene *scene, uint32_t width, uint32_t height, const rg_ambient *ambient,
                                  uint8_t *rgba_dev, float *rgb_dev, float *ao_dev, void *stream, rg_stats *stats);

#ifdef __cplusplus
}
#endif

#endif /* RAINGUN_H */
