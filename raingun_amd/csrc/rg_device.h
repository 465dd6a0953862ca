// rg_device.h — device-side scene layout shared by the render kernels and the
// C-ABI host code in rg_capi.hip.  gfx950 only.
//
// HBM layout of an uploaded scene (one rg_scene per device):
//   * hot tables (read by every ray, wave-uniform index -> scalar loads through
//     the constant address space, SGPR operands straight into v_*_f64):
//       sph[n_sph]   {cx, cy, cz, r*r}                 32 B  (bodies.rs:92-97)
//       sph_cc[n_sph] (cx*cx + cy*cy) + cz*cz           8 B   primary-ray shortcut
//       pln[n_pln]   {ox,oy,oz, nx,ny,nz, o.n, -}       64 B  (bodies.rs:136-149)
//       dsk[n_dsk]   {ox,oy,oz, nx,ny,nz, r, o.n}       64 B  (bodies.rs:173-192)
//       box[n_box]   {lo.xyz, hi.xyz}                   48 B  (bodies.rs:242-282)
//     each with an int id table giving the body's index in YAML order (the
//     closest-hit tie-break of scene.rs:34-39 is "first minimum in list order").
//   * cold tables (per-lane gathers at shading time, L2 resident):
//       bodies[n] {kind, params[7]}, mats[n] (one material per body),
//       lights[n_lights], textures (RGBA8 texels, one u32 per texel).
#pragma once
#include <stdint.h>

#if !defined(__HIP__) && !defined(__HIPCC__)  // plain C++ (host-only builds and tests of rg_bvh.cpp)
#define __device__
#define __host__
#define __forceinline__ inline
#endif

// Hot tables are read through the constant address space (addrspace 4) in
// device code: with a wave-uniform index that always lowers to s_load_* (SGPR
// operands, scalar cache), never to per-lane vector loads.
#ifdef __HIP_DEVICE_COMPILE__
#define RG_CONST __attribute__((address_space(4)))
#else
#define RG_CONST
#endif
template <class T>
__device__ __forceinline__ const RG_CONST T *rg_cptr(const T *p) { return (const RG_CONST T *)p; }

struct alignas(16) RgSph { double cx, cy, cz, r2; };
// f32 pre-filter records (see rg_k_intersect.h, "f32 pre-filter"): conservative
// bounds, never values the exact test uses.
struct alignas(16) RgSphF { float cx, cy, cz, r2hi; };       // c rounded to f32; r2 rounded up (+slack)
struct alignas(16) RgSphF2 { float cchi, thrp, cc32; int32_t id; };  // |c|^2 rounded up; primary-ray threshold; fl32(c.c); YAML body id (= sph_id)
struct alignas(16) RgPln { double ox, oy, oz, nx, ny, nz, on, pad; };
struct alignas(16) RgDsk { double ox, oy, oz, nx, ny, nz, r, on; };
struct alignas(16) RgBox { double lo[3], hi[3]; };

// 4-wide BVH over the sphere table (built on the host, rg_bvh.cpp).  Child
// boxes are f32, inflated and rounded outward so that the f32 slab test can
// only err towards "visit" (derivation: rg_k_bvh.h, "BVH traversal").
// child[k] >= 0: internal node; child[k] < 0: leaf, v = ~child[k], spheres
// [v >> 3, (v >> 3) + (v & 7) + 1) of the (BVH-ordered) sphere tables.
struct alignas(16) RgBvhNode {
    float lox[4], loy[4], loz[4], hix[4], hiy[4], hiz[4];
    int32_t child[4];
    int32_t nchild;        // valid children (2..4)
    int32_t pad[3];
};

// Per-lane traversal (incoherent rays, rg_k_bvh.h "bvh_lane") walks the
// same 4-wide nodes with a per-lane stack in LDS.  Stack entry: the f32 bits
// of the child's entry distance with the low RG_LANE_NODE_BITS cleared (a
// lower bound, so pruning at pop is conservative) | the child's node index.
#define RG_LANE_NODE_BITS 12
#define RG_LANE_STACK_MAX 16      // entries per lane the LDS arena may hold

struct RgBodyDev {         // per body, YAML order
    int32_t kind;
    int32_t pad;
    double p[7];
};

struct RgMatDev {          // material.rs:7-12 (+ Coloration 20-24, Surface 49-54), flattened
    int32_t coloration;
    float color[3];
    int32_t tex;
    float xoff, yoff;
    float albedo_pi;       // albedo / f32::consts::PI (rendering.rs:164), the host's f32 division
    int32_t surface;
    float reflectivity;
    float index;
    float transparency;
};

struct RgLightDev {        // lights.rs:8-26
    int32_t kind;
    float color[3];
    float intensity;
    int32_t pad;
    double v[3];              // direction (Directional) or position (Spherical)
    double dn[3];             // Directional: normalize(-direction) (lights.rs:48), a per-light constant
    double pad2;              // 80 B: 16-B multiple for LDS staging
};

struct RgLightBufDev;  // rg_lightbuf_ray.h

struct RgTexDev {
    const uint32_t *texels;  // RGBA8 packed little-endian: r | g<<8 | b<<16 | a<<24
    int32_t w, h;
};

// PLAIN light kernels only (rg_k_shade.h), made by the host once per scene.
struct RgTexMagic {        // per texture: the magic (rg_exact.h rg_magic_u32) of its width and of its height
    uint32_t mw, shw, mh, shh;
};
struct RgPlnAxes {         // per body id, planes only (else zero): the texture axes of bodies.rs:155-169
    double xa[3], ya[3];
};

// Everything a render launch needs, passed by value as the kernel argument.
struct RgKernelArgs {
    // hot tables
    const RgSph *sph;
    const double *sph_cc;
    const RgSphF *sphf;
    const RgSphF2 *sphf2;
    const int32_t *sph_id;
    const RgPln *pln;
    const int32_t *pln_id;
    const RgDsk *dsk;
    const int32_t *dsk_id;
    const RgBox *box;
    const int32_t *box_id;
    int32_t n_sph, n_pln, n_dsk, n_box;
    // BVH over the spheres (n_nodes == 0: none; brute-force sphere loops)
    const RgBvhNode *nodes;
    int32_t n_nodes;
    int32_t lane_stack;      // per-lane traversal stack entries (0: every lane walks wave-coherently)
    int32_t lane_min_depth;  // rays at this recursion depth or deeper walk per lane (if lane_stack > 0)
    float bvh_obound;        // near-ray origin bound |o_k| (rg_bvh_ray.h)
    double bvh_rbound;       // far rays: half-size of the region holding every inflated sphere box
    double bvh_margin;       // box inflation m
    double bvh_extent;       // S: max |coordinate| of any sphere bound
    // cold tables
    const RgBodyDev *bodies;
    const RgMatDev *mats;
    const RgLightDev *lights;
    const RgTexDev *texs;
    int32_t n_bodies, n_lights, n_textures;
    // LDS arena (byte offsets; used by the LDS-staged kernel variants)
    // [lane stacks | sphf | sphf2 | sph | cc | nodes | pln | dsk | box | bodies | mats | lights | texs] (byte offsets)
    uint32_t lds_lstack_bytes;  // per-lane traversal stacks at offset 0: lane_stack x block threads x 4 B
    uint32_t lds_sphf, lds_sph, lds_cc, lds_nodes, lds_pln, lds_dsk, lds_box, lds_bodies, lds_mats, lds_lights, lds_texs, lds_hot_bytes, lds_total_bytes;
    int32_t path;            // RG_PATH_* forced by rg_debug_set_path, or RG_PATH_AUTO
    // frame
    uint32_t width, height;
    uint32_t tile_rows, tile_stride, tile_offset, out_rows;
    // selected tiles in groups of tile_group consecutive image tiles (1: the plain round robin):
    // selected tile i is image tile (i / group) * stride + offset + i % group -- rank 0's larger
    // share of the N-rank frame loop (rg_frames_set_root_tiles)
    uint32_t tile_group;
    uint32_t tile_base;      // the launch renders selected tiles tile_base, tile_base + 1, ... (output row 0 = its first row)
    double fov_adjustment;   // tan(fov.to_radians() / 2), ray.rs:45 (host libm)
    double aspect;           // width / height, ray.rs:43
    float def[3];            // scene.default_color
    uint32_t max_depth;      // scene.max_recursion_depth
    // outputs
    uint32_t *rgba;          // packed RGBA8, out_rows * width
    float *rgb;              // nullable, out_rows * width * 3
    const uint32_t *tile_perm;     // nullable: dequeue order of the 8x8 tiles (expensive first)
    unsigned long long *counters;  // [0]=primary [1]=shadow [2]=secondary [3]=~error key [16+16q]=tile queue heads (RG_COUNTER_WORDS words)
    unsigned long long *counters_next;  // nullable: the other counter set of the launch context, zeroed by the render kernel
    // frames of the shading tree for depths above the compiled arrays (rg_k_frames.h FrameStack<0>)
    void *deep_stack;        // grid threads x (max_depth - 1) frames, frame i of thread g at [i * deep_stride + g]
    uint32_t deep_stride;    // threads of the grid the buffer was sized for
    int32_t nan_scene;       // a body or light parameter is non-finite or >= 1e100: NaN distances possible
    unsigned long long *err_sticky;  // nullable: the launch context's error word that survives launches
    // nullable: one word per 8x8 tile of the launch; when a wave has written a
    // tile (rgba in page-locked host memory) it stores frame_seq there after a
    // system-scope release, so the host can consume the tile's rows while the
    // kernel renders on (host-visible frames into pageable memory, streaming)
    uint32_t *tile_flags;
    uint32_t frame_seq;
    const uint32_t *cancel;  // nullable (host memory): nonzero = take no further tiles (streaming cancellation)
    // Tile shape: 64 pixels (a lane each), 2^tile_wlog wide and 64 >> tile_wlog
    // tall -- 3: 8x8 (default: ray coherence); 5: 32x2 and 6: 64x1 give whole
    // 128/256-B row segments per store, which PCIe writes into host memory need
    // (8x8 tiles finishing in scattered order: 29.6 GB/s, 32x2: 51-53, 64x1:
    // 55-56; profiles/r02/host_visible/d2h_probe.jsonl)
    uint32_t tile_wlog;
    uint32_t defer_px;  // 1: hold pixels in LDS, one store per finished tile (the frame is in host memory)
    // nullable: the primary rays' sensor coordinates (ray.rs:46-51) per image
    // column (prim_sx[x]) and row (prim_sy[y]), computed on the host with the
    // kernel's exact expressions -- two f64 divisions per pixel become two loads
    const double *prim_sx, *prim_sy;
    // 1: this launch is one of several frames in flight (rg_render_tiles_async):
    // the heavy path sizes its persistent grid for throughput, not latency (rg_render_grid.h)
    uint32_t pipelined;
    // (double)width, (double)height (ray.rs:46-51 divisions): kernel arguments land in SGPRs,
    // where the kernel's own conversions would hold two loop-invariant VGPR pairs
    double width_d, height_d;
    // nullable, host memory the device can write: the last wave of the launch to finish copies
    // the 4 statistics words (rays by class, error key) there -- no copy after the kernel
    unsigned long long *snap_out;
    uint32_t max_grid_threads;  // nonzero: cap on the persistent grid (the deep frame buffer's memory bound)
    // 1 (host-frame launches only): rgba is the WHOLE image and every pixel goes to its image row
    // (y * width + x) instead of its dense output row -- a device of rg_render_multi writes its
    // interleaved row tiles straight into the caller's frame (padding rows are not stored)
    uint32_t image_rows;
    // > 1: this launch is part j = out_tile_add of a call split into out_tile_mul launches (the
    // call's selected tile i -> launch i % mul); its selected tile s is written as the call's
    // tile s * mul + add, so the parts together fill the call's dense output
    uint32_t out_tile_mul, out_tile_add;
    // nullable: the whole LDS arena [0, lds_total_bytes) as one device image (light path): a
    // block stages its scene copy with ONE unrolled loop instead of a loop per table
    const void *lds_blob;
    // nullable: shadow-ray light buffers of the first n_lbuf lights (rg_lightbuf_ray.h); a light's
    // shadow rays test only the spheres of their cell's list (heavy path, BVH scenes)
    const RgLightBufDev *lbuf;
    const uint32_t *lb_start;  // cell list starts (per light: cells + 1 words, at RgLightBufDev::cell_off)
    const uint32_t *lb_ent;    // sphere positions of every list
    int32_t n_lbuf;
    int32_t lb_cam;            // >= 0: lbuf[lb_cam] is the camera buffer (a light buffer at the origin, primary rays)
    uint32_t lds_lbuf;         // LDS arena: the light-buffer descriptors (hot tables, after the texture descriptors)
    // light path into page-locked host memory (defer_px, LDS tile ring): finished tiles per ring flush
    // (1 .. RG_HOST_RING) and consecutive tiles the queue hands a wave at a time (1 .. ring_flush);
    // 0 = RG_HOST_RING for both.  Small launches (rg_render_multi's shares) want small groups (balance),
    // whole frames long runs of host memory per flush (rg_capi.hip host_ring_for)
    uint32_t ring_flush, ring_group;
    // Sparse launches (the SPARSE instantiations of rg_render_kernel only; adaptive anti-aliasing,
    // rg_aa.hip): px_mask non-null selects them.  The queue hands out tile_perm[0 .. tile_limit),
    // a LIST of the launch's 8x8 tiles, and a lane renders its pixel (x, y) only if
    // px_mask[(y / px_k) * px_w + x / px_k] is non-zero (one byte per px_k x px_k block of the
    // frame, px_w blocks per row); the other lanes store nothing and count no ray.  At the end of
    // the struct: the other instantiations keep their argument offsets.
    const uint8_t *px_mask;
    uint32_t tile_limit, px_k, px_w;
    // The PLAIN light kernels' camera quotients (rg_exact.h rg_recip_quot): 1.0 / width_d and
    // 1.0 / height_d.  plain_veto != 0: the launch runs the general kernel -- the residual form differs
    // from the division for some column or row of this frame size (bit 0; also set by
    // rg_debug_set_exact_div(0)), or there is no blob image (bit 1), or the launch has a camera (bit 2).
    // The launch context fills all three.
    uint32_t plain_veto;
    double inv_w, inv_h;
    // The PLAIN light kernels' tile start: the magic (rg_exact.h rg_magic_u32) of the launch's tiles per
    // row (8x8 tiles); log2 of tile_rows, or 32 where it is no power of two -- then its magic; and 1
    // where output row, image row and the call's row are one and the same (tile_stride 1, tile_offset 0,
    // tile_base 0, no groups, no split call), so that the kernel skips the mapping.
    uint32_t tiles_x_m, tiles_x_sh, tile_rows_shift, tile_rows_m, tile_rows_sh, rows_identity;
    // The PLAIN light kernels' two tables behind the arena [0, lds_total_bytes) in the blob image:
    // texm[n_textures] parallel to texs, axes[n_bodies] by body id; the arena with them is
    // [0, lds_plain_bytes), the LDS those kernels are launched with and stage.
    uint32_t lds_texm, lds_axes, lds_plain_bytes;
    // The launch's camera (rg_camera.h; rg_scene_set_camera), by value: camera != 0 selects the camera
    // family of rg_render_kernel (rg_render_cfg.h RG_MAXD_CAMERA), whose primary rays leave cam_eye
    // towards normalize((cam_right * sx + cam_up * sy) + cam_forward).  0: the reference's view from
    // the origin down -z, and the other members are not read.  At the end of the struct: the other
    // instantiations keep their argument offsets.
    uint32_t camera;
    double cam_eye[3], cam_right[3], cam_up[3], cam_forward[3];
    // nullable: the shadow mask volume (rg_shadow_vol.h; PLAIN light kernels only): shvol_g^3 words, the
    // word of a shadow origin's cell (rg_shadow_vol_cell.h rg_shvol_cell with shvol_inv, shvol_off) has
    // bit i set if sphere i, bit 16 + j if plane j could occlude a light from there.  Null: every body
    // is tested.  At the end of the struct: the other instantiations keep their argument offsets.
    const uint32_t *shvol;
    uint32_t shvol_g;
    float shvol_inv, shvol_off;
    // the struct grows by 32 bytes, so the arguments that follow it in other kernels (rg_trace_kernel,
    // rg_aov_kernel) keep their 16-byte phase and those kernels their code (profiles/shvol/kernel_isa_diff.txt)
    // first_hit_off, in the padding's first word so that no offset moves: nonzero = no tile takes the PLAIN
    // light kernels' first-hit path (rg_render_kernel.h; rg_debug_set_first_hit_tiles(0)) --
    // its vote fails in every wave
    union {
        uint32_t shvol_pad[3];
        uint32_t first_hit_off;
    };
    // The launch's thin lens (rg_lens.h; rg_scene_set_lens), by value: lens != 0 selects the lens family
    // of rg_render_kernel (rg_render_cfg.h RG_MAXD_LENS; a band of a supersampled frame with lens_k x lens_k
    // samples per pixel, rg_aa.hip), whose primary rays leave cam_eye + O for the point of the plane in
    // focus: lens_r / lens_u are normalize(cam_right / cam_up) * aperture, lens_tab the scene's device
    // table (RG_LENS_TABLE_DOUBLES doubles: every k's points, then the rotations).  Such a launch always
    // has camera != 0 (the identity camera where the scene has none).  0: the other members are not read.
    // At the end of the struct: the other instantiations keep their argument offsets; it grows by 80
    // bytes, a multiple of 16, for the reason shvol_pad gives.
    uint32_t lens, lens_k;
    double lens_focus, lens_r[3], lens_u[3];
    const double *lens_tab;
    // The launch's area lights (rg_area.h; rg_scene_set_light_radii), in the lens's padding so that no offset
    // moves and the struct keeps its size: area_tab, the scene's device table (every k's points, then the
    // radii, one per light), is at once the flag -- non-null selects the area family of rg_render_kernel
    // (rg_render_cfg.h RG_MAXD_AREA; a band of a supersampled frame with lens_k x lens_k samples per pixel),
    // whose every use of a spherical light's position takes the sample's point of the light's sphere, turned
    // by lens_tab + 2 * RG_LENS_POINTS.  Such a launch has camera != 0 (the identity camera where the scene
    // has none), takes the lens ray where lens != 0, and has no light buffers (lbuf null, n_lbuf 0, lb_cam -1).
    union {
        uint32_t lens_pad[2];
        const double *area_tab;
    };
};

__host__ __device__ inline uint32_t rg_tile_w(const RgKernelArgs &a) { return 1u << a.tile_wlog; }
__host__ __device__ inline uint32_t rg_tile_h(const RgKernelArgs &a) { return 64u >> a.tile_wlog; }
__host__ __device__ inline uint32_t rg_tiles_x(const RgKernelArgs &a) { return (a.width + rg_tile_w(a) - 1u) >> a.tile_wlog; }
__host__ __device__ inline uint32_t rg_tiles_y(const RgKernelArgs &a) { return (a.out_rows + rg_tile_h(a) - 1u) / rg_tile_h(a); }
__host__ __device__ inline unsigned long long rg_tile_count(const RgKernelArgs &a) {
    return (unsigned long long)rg_tiles_x(a) * rg_tiles_y(a);
}

// sizeof(Frame) in rg_k_frames.h (the deep frame buffer is sized on the host)
#define RG_FRAME_BYTES 88

// Light-path frames into page-locked host memory (the one-launch host-frame kernels' LDS tile ring,
// rg_render_kernel.h): finished tiles per ring flush and consecutive tiles per queue slot, for launches
// below RG_RING_BIG_TILES 64-pixel tiles (rg_render_multi's device shares: balance over the waves)
// and from it (whole frames, part B of split frames: long runs of host memory per flush).  test1 4K
// (profiles/r06/s5/hv_ring_sweep.out): 8-device rehearsal 0.2895 ms banded -> 0.207 ms one launch
// at 4 / 1 (16 / 16: 0.241, 4 / 4: 0.273); the 1-GPU pinned frame 0.805 -> 0.768 ms at 8 / 8.
#ifndef RG_RING_FLUSH_SMALL
#define RG_RING_FLUSH_SMALL 4
#endif
#ifndef RG_RING_GROUP_SMALL
#define RG_RING_GROUP_SMALL 1
#endif
#ifndef RG_RING_FLUSH_BIG
#define RG_RING_FLUSH_BIG 8
#endif
#ifndef RG_RING_GROUP_BIG
#define RG_RING_GROUP_BIG 8
#endif
#ifndef RG_RING_BIG_TILES
#define RG_RING_BIG_TILES 50000u
#endif
#ifndef RG_MULTI_LIGHT_ONE
#define RG_MULTI_LIGHT_ONE 1  // rg_render_multi, automatic mode: light scenes' shares as one launch per device
#endif
#ifndef RG_LB
#define RG_LB 3                   // lights per shadow batch on the light path (its LB template parameter)
#endif
#ifndef RG_LB_SMALL
#define RG_LB_SMALL 2             // light scenes with at most this many lights run a batch this wide (0: off)
#endif
#ifndef RG_LB_ONE
#define RG_LB_ONE 1               // light scenes with one light (or none) run a batch of one
#endif
// The PLAIN light kernels' shadow mask volume (rg_shadow_vol.h; 0: every body is tested and
// no volume is built, for A/B builds), and its two parts: the spheres' bits and the planes' bits.
#ifndef RG_PLAIN_SHVOL
#define RG_PLAIN_SHVOL 1
#endif
#ifndef RG_PLAIN_SHVOL_SPHERES
#define RG_PLAIN_SHVOL_SPHERES 1
#endif
#ifndef RG_PLAIN_SHVOL_PLANES
#define RG_PLAIN_SHVOL_PLANES 1
#endif
// The PLAIN light kernels' straight-line path for tiles whose primary rays all end at a miss or a hit
// that needs no secondary ray (rg_render_kernel.h; 0: every tile through the state
// machine, the parent's code, for A/B builds).
#ifndef RG_PLAIN_FIRST_HIT
#define RG_PLAIN_FIRST_HIT 1
#endif
#ifndef RG_HEAVY_WPS
#define RG_HEAVY_WPS 3            // heavy path: waves per SIMD (block = 256 * WPS threads; 168 VGPRs)
#endif
#define RG_BVH_MAX_WAVES 16       // waves per block on the BVH path (256 * RG_HEAVY_WPS threads): one rg_bvh_stack row each
#ifndef RG_HEAVY_SCENE_BODIES
#define RG_HEAVY_SCENE_BODIES 32  // bodies per ray at which the trace loop, not shading, dominates
#endif

#define RG_PATH_AUTO -1
#define RG_PATH_LIGHT 0   // 2 waves/SIMD, batched shadow rays, exact f64 tests only
#define RG_PATH_HEAVY 1   // 4 waves/SIMD, one ray per lane, f32 pre-filter + exact f64 tests

// Kernel path of a launch (the launcher and the host's tile-order policy agree on it).
__host__ __device__ __forceinline__ bool rg_heavy_path(const RgKernelArgs &a) {
    bool heavy = a.n_sph + a.n_pln + a.n_dsk + a.n_box >= RG_HEAVY_SCENE_BODIES;
    if (a.path != RG_PATH_AUTO) heavy = a.path == RG_PATH_HEAVY;
    if (a.n_lights > RG_LB) heavy = true;  // the light path shades all lights in ONE batch
    return heavy;
}

#define RG_COUNTER_WORDS (16 + 16 * 16 + 16)  // stats + 16 queue heads, 128 B apart + the finished-wave count
#define RG_DONE_WORD (16 + 16 * 16)            // waves of the launch that finished (RgKernelArgs::snap_out)
#define RG_FIRST_HIT_WORD (RG_DONE_WORD + 1)   // tiles of the launch that finished on the PLAIN kernels' first-hit path

// counters[3] holds ~((pixel << 8) | -status) of the lowest erroring pixel
// (atomicMax of the complement); 0 = no error, so one memset resets all four.
