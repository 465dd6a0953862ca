// rg_render_kernel.h — the render megakernel for gfx950 (MI355X).
//
// One lane = one pixel.  A wave renders 8x8 pixel tiles (ray coherence) taken
// from a sharded atomic queue.  The reference's recursion
//   render_pixel -> get_color -> {shade_diffuse | cast_ray -> get_color ...}
// (raingun-lib/src/rendering.rs:71-172) becomes a per-lane state machine:
// every loop iteration each live lane owns exactly ONE query ray (closest-hit
// or shadow) and all lanes of the wave walk the body tables together, with a
// wave-uniform body index, so body parameters come in through the scalar
// cache as SGPR operands and the only divergence is in shading.
//
// Post-order evaluation with an explicit frame stack reproduces the
// reference's f32 colour composition bit for bit (same operations, same
// order), so the RGBA8 output is byte-identical to the CPU restatement.
//
// Numerics: -ffp-contract=off (and the pragma below): every f64/f32 multiply
// and add is rounded separately, exactly as the reference's unfused Rust.
// Division and sqrt are the correctly-rounded hipcc expansions.
//
// The device code it is built from, one concern per header: rg_k_math.h, rg_k_intersect.h,
// rg_k_bvh.h, rg_k_trace.h, rg_k_shade.h, rg_k_frames.h, rg_k_pool.h; the RG_ITER_STATS
// counters: rg_k_diag.h.  What the template parameters mean, with every constant derived from
// them: rg_render_cfg.h.  Launch policy: rg_render_launch.h (grid: rg_render_grid.h), instantiated
// per frame-stack depth and path by rg_render_*.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/raingun.h"
#include "rg_camera.h"
#include "rg_device.h"
#include "rg_k_bvh.h"
#include "rg_k_diag.h"
#include "rg_k_frames.h"
#include "rg_k_intersect.h"
#include "rg_k_math.h"
#include "rg_k_pool.h"
#include "rg_k_shade.h"
#include "rg_k_trace.h"
#include "rg_area.h"
#include "rg_lens.h"
#include "rg_render_cfg.h"
#include "rg_shadow_vol_cell.h"

#pragma clang fp contract(off)

using namespace rgk;

// (the scheduling tunables the kernel's configuration is derived from: rg_render_cfg.h)
#ifndef RG_NQ
#define RG_NQ 8   // tile-queue heads (see the kernel's tile loop)
#endif
#define RG_QUEUE_BASE 16   // counters[16 + 16*q]: head q, one 128-B line each
#define RG_QUEUE_STRIDE 16
// What the PLAIN kernels do without the reference's divisions (0: as the other kernels, for
// A/B builds): the camera ray from host reciprocals and unscaled sqrt / reciprocal; the tile start
// from the host's magic of tiles per row, a shift for tile_rows and no row mapping where it is the
// identity.  (RG_PLAIN_WRAP and RG_PLAIN_AXES, the textured hit's two: rg_k_shade.h.)
#ifndef RG_PLAIN_CAMERA
#define RG_PLAIN_CAMERA 1
#endif
#ifndef RG_PLAIN_TILE
#define RG_PLAIN_TILE 1
#endif

// Per-launch view of the cold (shading) tables: LDS copies or global.
struct Cold {
    const RgBodyDev *bodies;
    const RgMatDev *mats;
    const RgLightDev *lights;
    const RgTexDev *texs;
};

// Stage [src, src+bytes) into LDS at dst (both 16-B aligned, bytes % 16 == 0).
__device__ __forceinline__ void stage16(unsigned char *dst, const void *src, uint32_t bytes) {
    uint4 *d = reinterpret_cast<uint4 *>(dst);
    const uint4 *g = reinterpret_cast<const uint4 *>(src);
    for (uint32_t k = threadIdx.x; k < bytes / 16u; k += blockDim.x) d[k] = g[k];
}

// Light l as the ray tree of sample-frame pixel `pix` sees it -- the ONE place the kernel reads a light, so that
// direction, distance and intensity at every site agree.  The area family (K::area): a spherical light at this
// sample's point of its sphere (rg_area.h; pix = Y * a.width + X with Y the row of the whole sample frame, for a
// fan helper or a pool task the OWNER's pixel), by value; every other kernel: a reference to the table's entry,
// as if it read it in place -- its code is the code it had.
template <class K>
__device__ __forceinline__ decltype(auto) light_at(const RgKernelArgs &a, const RgLightDev *lights, int l,
                                                   [[maybe_unused]] uint32_t pix) {
    if constexpr (K::area) {
        RgLightDev L = lights[l];
        if (L.kind != RG_LIGHT_DIRECTIONAL) {
            double pos[3];
            rg_area_position(L.v, a.area_tab[RG_AREA_POINT_DOUBLES + (uint32_t)l], pix % a.width, pix / a.width, a.lens_k,
                             a.width / a.lens_k, (uint32_t)l, a.area_tab + 3u * rg_lens_points_offset(a.lens_k),
                             a.lens_tab + 2u * RG_LENS_POINTS, pos);
            L.v[0] = pos[0];
            L.v[1] = pos[1];
            L.v[2] = pos[2];
        }
        return L;
    } else {
        return (lights[l]);
    }
}

// Render kernel.  Heavy path: ONE persistent block of 256*WPS threads per CU
// (WPS waves per SIMD).  Light path: one-wave blocks, each rendering at most
// RG_LIGHT_TILES_PER_WAVE tiles (grid: rg_render_grid.h).  A block stages the
// scene into LDS (LSPH: sphere, plane, disk and box tables, lights, texture
// descriptors; LCOLD: bodies, materials; LCOLD without LSPH: only the BVH nodes, after the per-lane
// walk stacks -- scenes whose sphere tables exceed the budget), then every wave repeatedly takes the next 8x8 pixel
// tile from an atomic queue (counters[16..], sharded) and runs the per-lane
// state machine until its 64 lanes have written their pixels.
// What the twelve parameters mean, and every fact derived from them (K:: below): rg_render_cfg.h.
// PLAIN (LDS-blob light kernels with array frames only): the launcher has checked (rg_render_launch.h
// rg_light_plain) that the scene has no disks and no boxes, that a.rgb, a.tile_perm and a.lbuf are null,
// that a.nan_scene is 0 and that a.n_lights == LB, so the kernel holds them as compile-time facts.
// It has also checked what lets a PLAIN kernel replace divisions by launch constants with exact forms
// (rg_exact.h): the camera quotients of this frame size, the camera ray's range, the blob image.
// MAXD == RG_MAXD_CAMERA (the camera family): the MAXD == 0 kernel whose primary rays leave
// a.cam_eye in the directions of rg_camera.h and are traced by the general closest-hit query.
// MAXD == RG_MAXD_LENS (the lens family): that kernel again, whose primary rays are the lens
// rays of rg_lens.h -- the one difference, at the RGR_PRIM site.
// MAXD == RG_MAXD_AREA (the area family): the lens family's kernel (the lens ray where a.lens, the
// camera ray otherwise) whose every light is read through light_at: a spherical light stands at the point of
// its sphere that rg_area.h gives the sample whose ray tree the lane is tracing.
// SPARSE (global frames only): the queue hands out the launch's tile LIST a.tile_perm[0 .. a.tile_limit) and a lane
// renders its pixel only where a.px_mask says so (adaptive anti-aliasing, rg_aa.hip; RgKernelArgs::px_mask).
template <int MAXD, bool LSPH, bool LCOLD, int WPS, int LBT, bool F32F, bool BVH, bool TASKS, int TPW = 0,
          bool HF = false, bool SPARSE = false, bool PLAIN = false>
__global__ __launch_bounds__(64 * rg_block_waves(LBT, WPS), rg_min_waves_per_eu(LBT, WPS))
void rg_render_kernel(RgKernelArgs a) {
    using K = RenderCfg<MAXD, LSPH, LCOLD, WPS, LBT, F32F, BVH, TASKS, TPW, HF, SPARSE, PLAIN>;
    constexpr int LB = K::lights_per_batch;  // shorthand: the per-light loops below are unrolled over it
    // PLAIN: the spherical lights' sqrt and 1.0 / m without their range scaling, per lane admitted
    // (rg_k_math.h sqrt_rcp_guarded)
    constexpr bool UL = PLAIN && RG_PLAIN_ULIGHT != 0;
    // PLAIN: a shaded hit looks up its shadow origin's word of the scene's shadow mask volume, the wave
    // ORs the words and trace_shadow walks the bodies left (rg_shadow_vol.h)
    constexpr bool SHV = PLAIN && RG_PLAIN_SHVOL != 0;
#ifdef RG_WAVE_TIMES  // diagnostic: per-wave start (before staging), staged, end (100 MHz ticks), tiles
    const unsigned long long t_wave0 = wall_clock64();
    uint32_t wt_tiles = 0;
#endif
    // what PLAIN fixes at compile time (the other kernels read the launch's arguments)
    const int n_lights = PLAIN ? LB : a.n_lights;
    const bool nan_scene = PLAIN ? false : a.nan_scene != 0;
    float *const out_rgb = PLAIN ? nullptr : a.rgb;
    const uint32_t *const tile_perm = PLAIN ? nullptr : a.tile_perm;
    // the launch context's other counter set (the previous launch's, read back
    // already: same stream) starts the next launch at zero -- no memset per frame
    if (blockIdx.x == 0 && a.counters_next)
        for (uint32_t k = threadIdx.x; k < RG_COUNTER_WORDS; k += blockDim.x) a.counters_next[k] = 0ull;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typename std::conditional<LSPH, SphLds, typename std::conditional<K::lds_nodes_only, SphNodesLds, SphScalar>::type>::type src;
    Cold T;
    // light path: every one-wave block stages its own copy of the (few-KB) scene; with the
    // arena's device image that is one loop with all its loads in flight at once
    const bool blob = K::light && LSPH && LCOLD && a.lds_blob != nullptr;
    if (blob) {
        const uint4 *g = reinterpret_cast<const uint4 *>(a.lds_blob);
        uint4 *d = reinterpret_cast<uint4 *>(smem);
        const uint32_t n16 = (PLAIN ? a.lds_plain_bytes : a.lds_total_bytes) / 16u;  // PLAIN: with its two tables
        // four loads in flight per lane: unconditional (indices clamped into the image), then
        // the guarded LDS stores -- no per-lane array, which hipcc placed in scratch
        const uint32_t last = n16 - 1u;
        for (uint32_t k0 = threadIdx.x; k0 < n16; k0 += 4u * blockDim.x) {
            const uint32_t k1 = k0 + blockDim.x, k2 = k1 + blockDim.x, k3 = k2 + blockDim.x;
            const uint4 v0 = g[k0], v1 = g[min(k1, last)], v2 = g[min(k2, last)], v3 = g[min(k3, last)];
            d[k0] = v0;
            if (k1 < n16) d[k1] = v1;
            if (k2 < n16) d[k2] = v2;
            if (k3 < n16) d[k3] = v3;
        }
    }
    if constexpr (LSPH) {
        if (!blob) {
        stage16(smem + a.lds_sphf, a.sphf, (uint32_t)a.n_sph * (uint32_t)sizeof(RgSphF));
        stage16(smem + a.lds_sphf + (size_t)a.n_sph * sizeof(RgSphF), a.sphf2, (uint32_t)a.n_sph * (uint32_t)sizeof(RgSphF2));
        stage16(smem + a.lds_sph, a.sph, (uint32_t)a.n_sph * (uint32_t)sizeof(RgSph));
        stage16(smem + a.lds_cc, a.sph_cc, a.lds_nodes - a.lds_cc);
        if constexpr (BVH) {
            stage16(smem + a.lds_nodes, a.nodes, (uint32_t)a.n_nodes * (uint32_t)sizeof(RgBvhNode));
        }
        stage16(smem + a.lds_pln, a.pln, (uint32_t)a.n_pln * (uint32_t)sizeof(RgPln));
        stage16(smem + a.lds_dsk, a.dsk, (uint32_t)a.n_dsk * (uint32_t)sizeof(RgDsk));
        stage16(smem + a.lds_box, a.box, a.lds_lights - a.lds_box);
        stage16(smem + a.lds_lights, a.lights, (uint32_t)a.n_lights * (uint32_t)sizeof(RgLightDev));
        stage16(smem + a.lds_texs, a.texs, a.lds_lbuf - a.lds_texs);
        if constexpr (!PLAIN)
            if (a.lbuf) stage16(smem + a.lds_lbuf, a.lbuf, a.lds_bodies - a.lds_lbuf);
        }
        src.f = reinterpret_cast<const RgSphF *>(smem + a.lds_sphf);
        src.f2 = reinterpret_cast<const RgSphF2 *>(smem + a.lds_sphf + (size_t)a.n_sph * sizeof(RgSphF));
        src.s = reinterpret_cast<const RgSph *>(smem + a.lds_sph);
        src.cc = reinterpret_cast<const double *>(smem + a.lds_cc);
        src.pl = reinterpret_cast<const RgPln *>(smem + a.lds_pln);
        src.dk = reinterpret_cast<const RgDsk *>(smem + a.lds_dsk);
        src.bx = reinterpret_cast<const RgBox *>(smem + a.lds_box);
        src.nd = reinterpret_cast<const RgBvhNode *>(smem + a.lds_nodes);
        src.lb = reinterpret_cast<const RgLightBufDev *>(smem + a.lds_lbuf);
        src.lt = reinterpret_cast<const RgLightDev *>(smem + a.lds_lights);
    } else {
        src.s = rg_cptr(a.sph);
        src.cc = rg_cptr(a.sph_cc);
        src.f = rg_cptr(a.sphf);
        src.f2 = rg_cptr(a.sphf2);
        src.pl = rg_cptr(a.pln);
        src.dk = rg_cptr(a.dsk);
        src.bx = rg_cptr(a.box);
        if constexpr (K::lds_nodes_only) {  // the nodes after the per-lane walk stacks
            stage16(smem + a.lds_lstack_bytes, a.nodes, (uint32_t)a.n_nodes * (uint32_t)sizeof(RgBvhNode));
            src.nd = reinterpret_cast<const RgBvhNode *>(smem + a.lds_lstack_bytes);
        } else {
            src.nd = rg_cptr(a.nodes);
        }
        src.lb = a.lbuf;
        src.lt = a.lights;
    }
    if constexpr (LSPH && LCOLD) {
        if (!blob) {
            stage16(smem + a.lds_bodies, a.bodies, (uint32_t)a.n_bodies * (uint32_t)sizeof(RgBodyDev));
            stage16(smem + a.lds_mats, a.mats, (uint32_t)a.n_bodies * (uint32_t)sizeof(RgMatDev));
        }
        T.bodies = reinterpret_cast<const RgBodyDev *>(smem + a.lds_bodies);
        T.mats = reinterpret_cast<const RgMatDev *>(smem + a.lds_mats);
    } else {
        T.bodies = a.bodies;
        T.mats = a.mats;
    }
    if constexpr (LSPH) {  // lights and texture descriptors: part of the hot tables
        T.lights = reinterpret_cast<const RgLightDev *>(smem + a.lds_lights);
        T.texs = reinterpret_cast<const RgTexDev *>(smem + a.lds_texs);
    } else {
        T.lights = a.lights;
        T.texs = a.texs;
    }
    // PLAIN: the texture dimensions' magics and the planes' texture axes, behind the arena in the blob
    // image (the launcher runs a PLAIN kernel only with the image: rg_launch.hip)
    [[maybe_unused]] const PlainTex PT{reinterpret_cast<const RgTexMagic *>(smem + a.lds_texm),
                                       reinterpret_cast<const RgPlnAxes *>(smem + a.lds_axes)};
    if (TASKS || LSPH || LCOLD) {
        if constexpr (TASKS) pool_init();
        __syncthreads();
    }

    const int lane = threadIdx.x & 63;
    // With the frame in host memory (a.defer_px) the wave's finished pixels
    // wait here until its whole tile is done, then go out as ONE coalesced
    // store per tile (flush_tile): every store is a PCIe write whose
    // acknowledgement the wave's next vmcnt wait would otherwise sit out once
    // per finishing lane.
    // (a host-frame feature, K::host_frames: the array kernels of device-resident renders go without)
    __shared__ uint32_t tile_px[K::tile_px_rows][64];
    uint32_t *my_px = &tile_px[K::host_frames ? threadIdx.x >> 6 : 0][lane];
    // Light path into page-locked host memory without tile publication: the
    // finished tiles of a wave collect in an LDS ring and go out RING at a time.
    // A store to host memory completes only after its PCIe round trip, and on
    // gfx9 every later `s_waitcnt vmcnt` (a texel load, a frame pop from the
    // global frame buffer) waits for it too: one flush per RING tiles instead of
    // one per tile.
    constexpr int RING = K::ring;
    __shared__ uint32_t ring_px[RING > 0 ? RG_LIGHT_BLOCK_WAVES : 1][RING > 0 ? RING : 1][64];
    __shared__ uint32_t ring_tile[RING > 0 ? RG_LIGHT_BLOCK_WAVES : 1][RING > 0 ? RING : 1];
    [[maybe_unused]] const uint32_t rw = RING > 0 ? (threadIdx.x >> 6) % RG_LIGHT_BLOCK_WAVES : 0u;
    [[maybe_unused]] uint32_t nring = 0;  // tiles waiting in the ring (wave-uniform)
    [[maybe_unused]] uint32_t grp_next = 0, grp_end = 0;  // the wave's group of consecutive tiles (ring mode)
    // Light path: a diffuse hit's shading factors wait in LDS while its shadow
    // batch is traced (field k of the lane at park[k][lane], conflict-free), so
    // that only the query's own state is held in VGPRs across the trace.
    constexpr int PK_PP = 0, PK_LIN = LB, PK_REFL = 2 * LB, PK_COL = 2 * LB + 1, PK_KIND = 2 * LB + 4,
                  PK_R = 2 * LB + 5, PK_N = 2 * LB + 6;
    __shared__ float park_lds[K::light ? RG_LIGHT_BLOCK_WAVES : 1][K::light ? PK_N : 1][64];
    float *park = &park_lds[K::light ? (threadIdx.x >> 6) % RG_LIGHT_BLOCK_WAVES : 0][0][lane];  // field k at park[64 k]
#ifdef RG_BVH_STATS
    if (lane < 16) rg_stat_lds[(threadIdx.x >> 6) % RG_BVH_MAX_WAVES][lane] = 0ull;
#endif
    [[maybe_unused]] const unsigned long long t_kernel = RG_CLOCK();
#ifdef RG_WAVE_TIMES
    const unsigned long long t_staged = wall_clock64();
#endif
    const uint32_t twlog = K::host_frames ? a.tile_wlog : 3u, twmask = (1u << twlog) - 1u, th = 64u >> twlog;
    const uint32_t tiles_x = (a.width + twmask) >> twlog;
    const uint32_t ntiles = tiles_x * ((a.out_rows + th - 1u) / th);
    const C3 def = c3(a.def[0], a.def[1], a.def[2]);
    const int max_depth = (int)a.max_depth;
    [[maybe_unused]] const bool use_ring = RING > 0 && a.defer_px;
    // the launch's ring flush size and queue group (RgKernelArgs::ring_flush / ring_group)
    [[maybe_unused]] const uint32_t ring_n = RING > 0 ? (a.ring_flush ? min(a.ring_flush, (uint32_t)(RING > 0 ? RING : 1)) : (uint32_t)RING) : 1u;
    [[maybe_unused]] const uint32_t ring_g = RING > 0 ? (a.ring_group ? min(a.ring_group, ring_n) : ring_n) : 1u;
    // store the ring's tiles: each lane its pixel of every tile (same index rule as the tile start)
    [[maybe_unused]] auto flush_ring = [&]() {
        for (uint32_t k = 0; k < nring; ++k) {
            const uint32_t tile = ring_tile[rw][k];
            const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
            const uint32_t x = (tx << twlog) + ((uint32_t)lane & twmask);
            const uint32_t orow = ty * th + ((uint32_t)lane >> twlog);
            if (x < a.width && orow < a.out_rows) {
                const uint32_t row = a.image_rows ? out_row_to_y(a, orow) : out_row_of(a, orow);
                if (row != 0xFFFFFFFFu) a.rgba[(size_t)row * a.width + x] = ring_px[rw][k][lane];
            }
        }
        if (a.tile_flags) {  // a consumer on the host: ONE system-scope release publishes the ring's tiles
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
            if ((uint32_t)lane < nring)
                __hip_atomic_store(&a.tile_flags[ring_tile[rw][lane]], a.frame_seq, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
        }
        nring = 0;
    };
    uint32_t n_prim = 0, n_shadow = 0, n_sec = 0;
    [[maybe_unused]] uint32_t n_first_hit = 0;  // (wave-uniform) tiles the wave finished on the first-hit path
    FrameStack<K::array_frames> stk;  // K::global_frames: field-major frames in a global buffer, no scratch array
    stk.init(a);

    // Sharded tile queue: RG_NQ heads, head q serving tiles q, q + RG_NQ, ... (one
    // 128-B line per head).  A single head saturates at ~88 dequeues/us
    // (MI355X_MICROARCH.md "dequeue"), i.e. ~1.5 ms for a 4K frame of 8x8 tiles.
    // The waves of a block start on head (block % RG_NQ) -- adjacent tiles per CU --
    // and move to the next head when theirs is drained (work stealing for the tail).
    uint32_t qi = blockIdx.x % RG_NQ, qtried = 0;
    // Lane state.  A lane holds one pixel of the wave's 8x8 tile, or (task
    // splitting, TASKS) one published subtree of another lane of the block;
    // the wave takes the next tile when none of its lanes has work.
    int mode = MODE_DONE;
    Ray q;                 // current query (shadow: q.o = shared origin)
    ShadowBatch<LB> sb;        // shadow: the batch's directions and light distances
    uint32_t occl_full = 0u;
    [[maybe_unused]] uint32_t shw = 0u;  // SHV: the batch's word of the shadow mask volume (set with the batch)
    int qdepth = 0;        // closest: depth of the ray
    // hit being shaded
    V3 hp = v3(0, 0, 0), hn = v3(0, 0, 0);
    int hb = 0, hdepth = 0, li = 0;
    int nfan = 0;              // shadow fan-out: lights li+1 .. li+nfan of this hit traced by helper lanes
    uint32_t fan_lanes = 0u;   // ... their lanes, 6 bits each
    uint32_t fan_bits = 0u;    // ... their occlusion results, bit k
    C3 fin = c3(0, 0, 0), bcol = c3(0, 0, 0), ret = def;
    int sp = 0;
    Closest c;
    closest_init(c);
    bool have_result = false;  // c / occl hold a fresh result for the lane's query
    uint32_t occl = 0u;
    size_t oidx = 0;           // output index of the lane's pixel
    uint32_t pixel = 0;        // image pixel index (error reports) of the lane's pixel or task
    int task = -1;             // pool slot whose subtree this lane computes (-1: its own pixel)
    bool tiles_left = true;    // the tile queue has not been found empty
    [[maybe_unused]] uint32_t pf_k = 0u;       // lane 0: the prefetched slot of head qi (tile-slot prefetch)
    [[maybe_unused]] bool pf_valid = false;    // (wave-uniform) a slot is claimed
    uint32_t my_tile = 0xFFFFFFFFu;  // the wave's current tile (published when done: a.tile_flags)
    [[maybe_unused]] uint32_t tiles_taken = 0;
    [[maybe_unused]] bool counted = false;  // this wave is counted in pool_of().busy
#ifdef RG_TILE_TIMES
    uint32_t cur_tile = 0xFFFFFFFFu;  // diagnostic: per-tile time into rgb[tile] (us), wave iterations
    unsigned long long t_tile = 0, t_query = 0;  // into rgb[ntiles + tile], start, query time
    uint32_t tile_iters = 0;
#endif
    for (;;) {
        RG_REGION(RGR_LOOP);
        if constexpr (K::shadow_fan) {
            // shadow fan-out, collect: the helpers' occlusion bits (every lane active here)
            if (__any(nfan > 0)) {
                fan_bits = 0u;
#pragma unroll
                for (int k = 0; k < RG_SHADOW_FAN; ++k) {
                    const uint32_t b = (uint32_t)__shfl((int)occl, (int)((fan_lanes >> (6 * k)) & 63u), 64);
                    if (k < nfan) fan_bits |= (b & 1u) << k;
                }
            }
            if (mode == MODE_SHADOW_H) {  // a helper is idle again
                mode = MODE_DONE;
                have_result = false;
            }
        }
        if (have_result) {
            bool unwind = false;
            bool shade = false;           // run a shade_diffuse step this iteration
            const int rmode = mode;       // kind of result the lane holds
            if (TASKS && rmode == MODE_WAIT) {
                unwind = true;  // poll the awaited subtree (top frame FR_REFR_WAIT)
            } else if (rmode == MODE_CLOSEST) {
                if (c.nan && c.nhit >= 2) raise_error(a, pixel, RG_ERR_NAN_DISTANCE);
                if (c.id < 0) {
                    ret = def;  // rendering.rs:76-77, 128-129
                    unwind = true;
                } else {
                    // get_color (rendering.rs:80-120)
                    const RgBodyDev b = T.bodies[c.id];
                    const RgMatDev m = T.mats[c.id];
                    RG_REGION(RGR_GETCOLOR);
                    if (b.kind == RG_BODY_SPHERE) RG_REGION(RGR_NORMAL_SPHERE);
                    V3 h = add(q.o, scl(q.d, c.t));
                    V3 n;
                    if (!surface_normal(b, h, n)) raise_error(a, pixel, RG_ERR_AABB_NORMAL);
                    if (m.surface != RG_SURFACE_REFRACTIVE) {
                        if constexpr (K::light) {
                            // ONE batch covers every light (n_lights <= LB on this path): set it
                            // up now, with the per-light shading factors (parked in LDS), so that
                            // no hit-point state (h, n, incident) has to survive the shadow pass
                            // a textured hit's texel load goes out now and is converted after the
                            // lights' setup below (its latency overlaps that work: test1 0.2979 ->
                            // 0.2955 ms over 200 frames, profiles/r04/s15/session.txt)
                            const bool textured = m.coloration != RG_COLORATION_COLOR;
                            uint32_t texel = 0u;
                            RG_REGION(RGR_BATCH);
#ifdef RG_REGION_STATS
                            if (textured) {
                                RG_REGION(RGR_TEXEL);
                                if (b.kind == RG_BODY_SPHERE) RG_REGION(RGR_UV_SPHERE);
                                else if (b.kind != RG_BODY_AABB) RG_REGION(RGR_UV_PLANE);
                            }
#endif
                            if (textured) texel = PLAIN ? texel_fetch_plain(T.texs, PT, m, b, c.id, h) : texel_fetch(T.texs, m, b, h);
                            else { park[64 * PK_COL] = m.color[0]; park[64 * (PK_COL + 1)] = m.color[1]; park[64 * (PK_COL + 2)] = m.color[2]; }
                            park[64 * PK_REFL] = m.albedo_pi;                       // rendering.rs:164
                            // how the batch's colour is used: 0 diffuse, 1 reflecting at the depth
                            // limit (mix with the default colour), 2 reflecting with a frame
                            const int kind = m.surface == RG_SURFACE_DIFFUSE ? 0 : qdepth + 1 < max_depth ? 2 : 1;
                            park[64 * PK_KIND] = __int_as_float(kind);
                            park[64 * PK_R] = m.reflectivity;
                            // the shadow rays' origin hit + n*bias (rendering.rs:148) is also the
                            // reflection ray's origin (ray.rs:57): q.o serves both, and q.d (unused
                            // by the shadow pass) carries the reflection direction until the
                            // batch is shaded -- the frame holds only colour state
                            q.o = add(h, scl(n, SHADOW_BIAS));
                            if constexpr (SHV) {
                                // the origin's word of the shadow mask volume: one load, behind the texel's,
                                // read when the wave forms its mask (an origin without a cell: every body)
                                shw = RG_SHVOL_ALL;
                                if (a.shvol) {  // (wave-uniform)
                                    const int cell = rg_shvol_cell((float)q.o.x, (float)q.o.y, (float)q.o.z, a.shvol_inv,
                                                                   a.shvol_off, (int)a.shvol_g);
                                    const uint32_t w = a.shvol[cell >= 0 ? cell : 0];
                                    if (cell >= 0) shw = w;
                                }
                            }
                            // (rendering.rs:88: its frame is pushed once the batch is shaded)
                            if (kind == 2) q.d = sub(q.d, scl(n, 2.0 * dot(q.d, n)));  // ray.rs:58
                            occl_full = 0u;
#pragma unroll
                            for (int l = 0; l < LB; ++l) {
                                if (l < n_lights) {
                                    const RgLightDev L = light_at<K>(a, T.lights, l, pixel);
                                    if (L.kind != RG_LIGHT_DIRECTIONAL) RG_REGION(RGR_LIGHT_SPH);
                                    light_dir_dist<UL>(L, h, sb.d[l], sb.ld[l]);
                                    park[64 * (PK_PP + l)] = fmaxf((float)dot(n, sb.d[l]), 0.0f);  // rendering.rs:161-162
                                    park[64 * (PK_LIN + l)] = light_intensity(L, h);               // pure; used if lit
                                    occl_full |= 1u << l;
                                    n_shadow++;
                                } else {
                                    sb.d[l] = v3(0.0, 0.0, 1.0);
                                    sb.ld[l] = 0.0;
                                }
                            }
                            if (textured) {
                                const C3 col = texel_color(texel);
                                park[64 * PK_COL] = col.r; park[64 * (PK_COL + 1)] = col.g; park[64 * (PK_COL + 2)] = col.b;
                            }
                            if (n_lights > 0) mode = MODE_SHADOW;
                            else shade = true;  // no lights: finish with black (rendering.rs:138)
                        } else {
                            bcol = surface_color(T.texs, m, b, h);
                            hb = c.id; hdepth = qdepth;
                            fin = c3(0.0f, 0.0f, 0.0f);
                            hp = h; hn = n; li = 0;
                            // a reflecting hit's reflection direction (ray.rs:58) goes into q.d
                            // now -- the shadow queries use q.o and sb only -- so the incident
                            // direction does not stay live across the light loop
                            if (m.surface == RG_SURFACE_REFLECTING && qdepth + 1 < max_depth)
                                q.d = sub(q.d, scl(n, 2.0 * dot(q.d, n)));
                            shade = true;
                        }
                    } else {
                        RG_REGION(RGR_REFRACT);
                        float kr = (float)fresnel(q.d, n, m.index);
                        C3 surf = PLAIN ? surface_color_plain(T.texs, PT, m, b, c.id, h) : surface_color(T.texs, m, b, h);
                        int cd = qdepth + 1;
                        if (cd >= max_depth) {
                            // the transmission ray's unwrap (rendering.rs:106) precedes cast_ray's depth test
                            Ray tr;
                            if (kr < 1.0f && !transmission(n, q.d, h, m.index, tr)) raise_error(a, pixel, RG_ERR_TRANSMISSION);
                            C3 col = cadd(cscl(def, kr), cscl(def, 1.0f - kr));
                            ret = cmul(cscl(col, m.transparency), surf);
                            unwind = true;
                        } else {
                            RG_REGION(RGR_PUSH_REFR);  // frame writes: 18 dwords per lane (kr .. surf, pending ray, type)
                            auto &&f = stk[sp++];
                            f.f[0] = kr; f.f[1] = m.transparency;
                            f.f[2] = surf.r; f.f[3] = surf.g; f.f[4] = surf.b;
                            if constexpr (TASKS) f.cdepth = cd;
                            // rendering.rs:100-113: the transmission subtree is traced first while
                            // the reflection ray (ray.rs:56-60) waits in the frame or, with task
                            // splitting, is published so an idle lane of the block can trace it now
                            bool trace_t = false;
                            if (kr < 1.0f) {
                                if constexpr (TASKS) {
                                    Ray tr;
                                    if (transmission(n, q.d, h, m.index, tr)) {
                                        trace_t = true;
                                        const Ray rr = reflection(n, q.d, h);
                                        const int slot = pool_alloc(lane);
                                        if (slot >= 0) {
                                            double *pr = pool_of().ray[slot];
                                            pr[0] = rr.o.x; pr[1] = rr.o.y; pr[2] = rr.o.z;
                                            pr[3] = rr.d.x; pr[4] = rr.d.y; pr[5] = rr.d.z;
                                            pool_of().depth[slot] = cd;
                                            pool_of().pix[slot] = pixel;
                                            pool_publish(slot);
                                            f.type = FR_REFR_TASK | (slot << 8);
                                        } else {
                                            f.type = FR_REFR_T;
                                            f.rr[0] = rr.o.x; f.rr[1] = rr.o.y; f.rr[2] = rr.o.z;
                                            f.rr[3] = rr.d.x; f.rr[4] = rr.d.y; f.rr[5] = rr.d.z;
                                        }
                                        q = tr;
                                    }
                                } else {
                                    // the reflection ray goes to the frame BEFORE the transmission ray
                                    // is built (into q, written only on success): fewer live values
                                    const Ray rr = reflection(n, q.d, h);
                                    f.rr[0] = rr.o.x; f.rr[1] = rr.o.y; f.rr[2] = rr.o.z;
                                    f.rr[3] = rr.d.x; f.rr[4] = rr.d.y; f.rr[5] = rr.d.z;
                                    f.type = FR_REFR_T;
                                    trace_t = transmission(n, q.d, h, m.index, q);
                                }
                                if (!trace_t) raise_error(a, pixel, RG_ERR_TRANSMISSION);
                            }
                            if (!trace_t) {  // kr >= 1 (or the transmission panic): refraction colour = default
                                f.type = FR_REFR_R;
                                f.f[5] = def.r; f.f[6] = def.g; f.f[7] = def.b;
                                q = reflection(n, q.d, h);
                            }
                            qdepth = cd;
                            mode = MODE_CLOSEST;
                            n_sec++;
                        }
                    }
                }
            } else if (rmode == MODE_SHADOW) {
                shade = true;  // a shadow result for light li
            }
            if constexpr (K::light) {
              if (shade) {
                RG_REGION(RGR_SHADE);
                // shade_diffuse accumulation over the batch (rendering.rs:141-170), in light order
                const C3 bc = c3(park[64 * PK_COL], park[64 * (PK_COL + 1)], park[64 * (PK_COL + 2)]);
                const float refl = park[64 * PK_REFL];
                C3 acc = c3(0.0f, 0.0f, 0.0f);
#pragma unroll
                for (int l = 0; l < LB; ++l) {
                    if (l < n_lights) {
                        const RgLightDev L = light_at<K>(a, T.lights, l, pixel);
                        const float inten = !((occl >> l) & 1u) ? park[64 * (PK_LIN + l)] : 0.0f;
                        const float power = park[64 * (PK_PP + l)] * inten;
                        C3 lc = cscl(cscl(c3(L.color[0], L.color[1], L.color[2]), power), refl);
                        acc = cadd(acc, cmul(bc, lc));
                    }
                }
                C3 dcol = cclamp(acc);
                const int kind = __float_as_int(park[64 * PK_KIND]);
                if (kind == 0) {  // Diffuse
                    ret = dcol;
                    unwind = true;
                } else {  // Reflecting (rendering.rs:86-91)
                    if (kind == 1) {  // the reflection ray would be at depth >= max (rendering.rs:123-124)
                        const float r = park[64 * PK_R];
                        ret = cadd(cscl(dcol, 1.0f - r), cscl(def, r));
                        unwind = true;
                    } else {
                        RG_REGION(RGR_PUSH_REFL);  // frame writes: 5 dwords per lane (D.rgb, r, type)
                        auto &&f = stk[sp++];  // rendering.rs:88
                        f.type = FR_REFL;
                        f.f[0] = dcol.r; f.f[1] = dcol.g; f.f[2] = dcol.b; f.f[3] = park[64 * PK_R];
                        // q = the reflection ray (origin = the shadow origin, direction set at the hit)
                        // without task splitting the stack index is the depth; a lane tracing a pooled
                        // subtree starts at sp = 0 with a non-zero depth, so TASKS keeps the hit's depth
                        qdepth = TASKS ? qdepth + 1 : sp;
                        mode = MODE_CLOSEST;
                        n_sec++;
                    }
                }
              }
            } else if (shade) {
                // shade_diffuse loop body (rendering.rs:141-170), one light per iteration
                const RgMatDev m = T.mats[hb];
                if (rmode == MODE_SHADOW) {
                    const float refl = m.albedo_pi;  // albedo / PI (rendering.rs:164)
#pragma unroll
                    for (int l = 0; l < LB; ++l) {
                        if (li + l < a.n_lights) {
                            const RgLightDev L = light_at<K>(a, T.lights, li + l, pixel);
                            float inten = !((occl >> l) & 1u) ? light_intensity(L, hp) : 0.0f;
                            float power = fmaxf((float)dot(hn, sb.d[l]), 0.0f) * inten;
                            C3 lc = cscl(cscl(c3(L.color[0], L.color[1], L.color[2]), power), refl);
                            fin = cadd(fin, cmul(bcol, lc));
                        }
                    }
                    if constexpr (K::shadow_fan) {
                        // the lights helper lanes traced, in light order (rendering.rs:141-170)
                        for (int k = 0; k < nfan; ++k) {
                            const RgLightDev L = light_at<K>(a, T.lights, li + 1 + k, pixel);
                            V3 ldir;
                            double ldist;
                            light_dir_dist<UL>(L, hp, ldir, ldist);  // as at setup: same bits
                            float inten = !((fan_bits >> k) & 1u) ? light_intensity(L, hp) : 0.0f;
                            float power = fmaxf((float)dot(hn, ldir), 0.0f) * inten;
                            C3 lc = cscl(cscl(c3(L.color[0], L.color[1], L.color[2]), power), refl);
                            fin = cadd(fin, cmul(bcol, lc));
                        }
                        li += nfan;
                        nfan = 0;
                    }
                    li += LB;
                }
                if (li < a.n_lights) {
                    q.o = add(hp, scl(hn, SHADOW_BIAS));  // rendering.rs:148
                    occl_full = 0u;
#pragma unroll
                    for (int l = 0; l < LB; ++l) {
                        if (li + l < a.n_lights) {
                            light_dir_dist<UL>(light_at<K>(a, T.lights, li + l, pixel), hp, sb.d[l], sb.ld[l]);
                            occl_full |= 1u << l;
                            n_shadow++;
                        } else {
                            sb.d[l] = v3(0.0, 0.0, 1.0);
                            sb.ld[l] = 0.0;
                        }
                    }
                    mode = MODE_SHADOW;
                } else {
                    C3 dcol = cclamp(fin);
                    if (m.surface == RG_SURFACE_DIFFUSE) {
                        ret = dcol;
                        unwind = true;
                    } else {  // Reflecting (rendering.rs:86-91)
                        float r = m.reflectivity;
                        int cd = hdepth + 1;
                        if (cd >= max_depth) {
                            ret = cadd(cscl(dcol, 1.0f - r), cscl(def, r));
                            unwind = true;
                        } else {
                            RG_REGION(RGR_PUSH_REFL);  // frame writes: 5 dwords per lane (D.rgb, r, type)
                            auto &&f = stk[sp++];
                            f.type = FR_REFL;
                            f.f[0] = dcol.r; f.f[1] = dcol.g; f.f[2] = dcol.b; f.f[3] = r;
                            q.o = add(hp, scl(hn, SHADOW_BIAS));  // ray.rs:57; q.d set at the hit
                            qdepth = cd;
                            mode = MODE_CLOSEST;
                            n_sec++;
                        }
                    }
                }
            }
            if (unwind) {
                RG_REGION(RGR_UNWIND);
                for (;;) {
                    RG_REGION(RGR_UNWIND_STEP);
                    if (sp == 0) {
                        bool handed = false;
                        if constexpr (TASKS) {
                            if (task >= 0) {  // a published subtree: hand its colour back
                                pool_finish(task, ret);
                                task = -1;
                                handed = true;
                            }
                        }
                        if (!handed) {
                            const uint32_t px = f32_to_u8(ret.r * 255.0f) | (f32_to_u8(ret.g * 255.0f) << 8) |
                                                (f32_to_u8(ret.b * 255.0f) << 16) | 0xFF000000u;
                            if (K::host_frames && a.defer_px) *my_px = px;
                            else a.rgba[oidx] = px;
                            if (KDiag::rgb_is_output && out_rgb) { out_rgb[3 * oidx] = ret.r; out_rgb[3 * oidx + 1] = ret.g; out_rgb[3 * oidx + 2] = ret.b; }
                        }
                        mode = MODE_DONE;
                        break;
                    }
                    auto &&f = stk[sp - 1];
                    if constexpr (TASKS) {
                        const int ftype = f.type & 0xFF;
                        if (ftype == FR_REFR_TASK || ftype == FR_REFR_WAIT) {
                            const int slot = f.type >> 8;
                            if (ftype == FR_REFR_TASK) {  // ret = the transmission subtree's colour
                                f.f[5] = ret.r; f.f[6] = ret.g; f.f[7] = ret.b;
                                if (pool_reclaim(slot)) {  // nobody took the reflection ray: trace it here
                                    const double *r = pool_of().ray[slot];
                                    q.o = v3(r[0], r[1], r[2]);
                                    q.d = v3(r[3], r[4], r[5]);
                                    pool_release(slot);
                                    f.type = FR_REFR_R;
                                    qdepth = f.cdepth;
                                    mode = MODE_CLOSEST;
                                    n_sec++;
                                    break;
                                }
                                f.type = FR_REFR_WAIT | (slot << 8);
                            }
                            if (!pool_done(slot)) {  // another lane is still tracing it
                                mode = MODE_WAIT;
                                break;
                            }
                            const C3 rc = c3(pool_of().col[slot][0], pool_of().col[slot][1], pool_of().col[slot][2]);
                            pool_release(slot);
                            const float kr = f.f[0];  // as FR_REFR_R below (rendering.rs:115-117)
                            C3 col = cadd(cscl(rc, kr), cscl(c3(f.f[5], f.f[6], f.f[7]), 1.0f - kr));
                            ret = cmul(cscl(col, f.f[1]), c3(f.f[2], f.f[3], f.f[4]));
                            sp--;
                            continue;
                        }
                    }
                    if (f.type == FR_REFL) {
                        ret = cadd(cscl(c3(f.f[0], f.f[1], f.f[2]), 1.0f - f.f[3]), cscl(ret, f.f[3]));
                        sp--;
                    } else if (f.type == FR_REFR_T) {
                        RG_REGION(RGR_UNWIND_REFRT);  // frame writes: 4 dwords per lane (Tc.rgb, type)
                        f.f[5] = ret.r; f.f[6] = ret.g; f.f[7] = ret.b;
                        f.type = FR_REFR_R;
                        q.o = v3(f.rr[0], f.rr[1], f.rr[2]);
                        q.d = v3(f.rr[3], f.rr[4], f.rr[5]);
                        qdepth = TASKS ? f.cdepth : sp;  // without tasks the stack index is the depth
                        mode = MODE_CLOSEST;
                        n_sec++;
                        break;
                    } else {  // FR_REFR_R (rendering.rs:115-117)
                        float kr = f.f[0];
                        C3 col = cadd(cscl(ret, kr), cscl(c3(f.f[5], f.f[6], f.f[7]), 1.0f - kr));
                        ret = cmul(cscl(col, f.f[1]), c3(f.f[2], f.f[3], f.f[4]));
                        sp--;
                    }
                }
            }
        }
        have_result = false;
        // every lane of the wave is done: its tile is complete (owners hold their pixels)
        if (K::host_frames && my_tile != 0xFFFFFFFFu && (a.defer_px || a.tile_flags) && !__any(mode != MODE_DONE)) {
            bool ringed = false;
            if constexpr (RING > 0) {
                if (use_ring) {
                    ring_px[rw][nring][lane] = *my_px;
                    if (lane == 0) ring_tile[rw][nring] = my_tile;
                    if (++nring == ring_n) flush_ring();
                    ringed = true;
                }
            }
            if (!ringed) flush_tile(a, oidx, *my_px, my_tile, lane);
            my_tile = 0xFFFFFFFFu;
        }
        // a wave with no live lane takes the next tile
        if (tiles_left && !__any(mode != MODE_DONE)) {
            RG_REGION(RGR_TILE_FETCH);
#ifdef RG_TILE_TIMES
            if (cur_tile != 0xFFFFFFFFu && lane == 0 && a.rgb) {
                a.rgb[cur_tile] = (float)(wall_clock64() - t_tile) * 0.01f;  // 100 MHz clock
                a.rgb[ntiles + cur_tile] = (float)tile_iters;
                a.rgb[2 * ntiles + cur_tile] = (float)(t_tile & 0xFFFFFFull);  // start, 24-bit ticks (exact in f32)
                a.rgb[3 * ntiles + cur_tile] = (float)t_query * 0.01f;
            }
            cur_tile = 0xFFFFFFFFu;
#endif
            uint32_t tile = 0xFFFFFFFFu;
            if constexpr (RING > 0) {  // the rest of the wave's group of consecutive tiles
                if (use_ring && grp_next < grp_end) tile = grp_next++;
            }
            if (K::host_frames && a.cancel) {  // streaming: the consumer stopped (rendering.rs:53-67 `.all` short-circuits)
                uint32_t cv = 0u;
                if (lane == 0) cv = __hip_atomic_load(a.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                if (__builtin_amdgcn_readfirstlane(__shfl((int)cv, 0, 64)) != 0) qtried = RG_NQ;
            }
            // ring mode: the queue hands out groups of RING consecutive tiles (one contiguous
            // run of host memory per ring flush: 4 KB with 64x1 tiles)
            const uint32_t qlimit = SPARSE ? a.tile_limit : (RING > 0 && use_ring) ? (ntiles + ring_g - 1) / ring_g : ntiles;
            // Tile-slot prefetch (light path, device-resident launches): the slot claimed at the
            // previous tile's start, so the atomic's round trip overlaps that tile (round 4, same
            // box, interleaved: test1 0.2972 -> 0.2939 ms over 200 frames, test3 0.2656 -> 0.2631:
            // profiles/r04/s21/session.txt, s22).  Not on the heavy path: a claimed tile waits
            // behind the wave's current (long) one, which lengthens the tail (north star +0.6 %);
            // nor in the light path's persistent single launches (persistent waves), for the same reason:
            // rg_render_multi's shares, whose waves ended by 84 us (p50) while claimed tiles still
            // started at 145 us (profiles/r05/s18, s26)
            if constexpr (K::slot_prefetch) {
                if (pf_valid) {  // the slot claimed at the previous tile's start
                    const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)pf_k, 0, 64));
                    const unsigned long long t = (unsigned long long)k * RG_NQ + qi;
                    if (t < qlimit) tile = (uint32_t)t;
                    else { qi = (qi + 1) % RG_NQ; ++qtried; }  // that head is drained
                    pf_valid = false;
                }
            }
            while (tile == 0xFFFFFFFFu && qtried < RG_NQ) {
                uint32_t k = 0;
                if (lane == 0) k = atomicAdd(reinterpret_cast<unsigned int *>(&a.counters[RG_QUEUE_BASE + RG_QUEUE_STRIDE * qi]), 1u);
                k = __builtin_amdgcn_readfirstlane(__shfl(k, 0, 64));
                // head q serves tiles q, q+NQ, q+2NQ, ...: the tiles in flight stay a
                // compact raster-order band of the frame, as with a single head (the slot
                // prefetch above uses the same slot -> tile rule)
                const unsigned long long t = (unsigned long long)k * RG_NQ + qi;
                if (t < qlimit) {
                    tile = (uint32_t)t;
                    if constexpr (RING > 0) {
                        if (use_ring) {
                            tile = (uint32_t)t * ring_g;
                            grp_next = tile + 1u;
                            grp_end = min(tile + ring_g, ntiles);
                        }
                    }
                    break;
                }
                qi = (qi + 1) % RG_NQ;
                ++qtried;
            }
            if (tile == 0xFFFFFFFFu) {
                tiles_left = false;
            } else {
                if constexpr (!K::persistent) {
                    // a wave renders at most that many tiles, so the grid
                    // drains through the hardware dispatcher wave (block) by wave
                    if (++tiles_taken >= K::tiles_per_wave) tiles_left = false;
                }
                if constexpr (K::slot_prefetch) {
                    // claim the wave's NEXT queue slot now: the atomic's round trip overlaps this
                    // tile's work instead of stalling the wave between tiles (the wave renders
                    // the claimed tile, or finds the head drained, at its next tile start)
                    if (tiles_left) {
                        if (lane == 0)
                            pf_k = atomicAdd(reinterpret_cast<unsigned int *>(&a.counters[RG_QUEUE_BASE + RG_QUEUE_STRIDE * qi]), 1u);
                        pf_valid = true;
                    }
                }
                if constexpr (SPARSE) tile = a.tile_perm[tile];  // the list entry
                else if (tile_perm) tile = tile_perm[tile];  // scheduling order only; every tile is rendered once
#ifdef RG_WAVE_TIMES
                ++wt_tiles;
#endif
                if constexpr (K::host_frames) my_tile = tile;
                constexpr bool fast_tile = PLAIN && RG_PLAIN_TILE != 0;
                const uint32_t ty = fast_tile ? rg_magic_div(tile, a.tiles_x_m, a.tiles_x_sh) : tile / tiles_x;
                const uint32_t tx = tile - ty * tiles_x;
#ifdef RG_TILE_TIMES
                cur_tile = tile;
                t_tile = wall_clock64();
                t_query = 0;
                tile_iters = 0;
#endif
                const uint32_t x = (tx << twlog) + ((uint32_t)lane & twmask);
                const uint32_t orow = ty * th + ((uint32_t)lane >> twlog);
                bool alive = x < a.width && orow < a.out_rows;
                uint32_t y;
                if (fast_tile && a.rows_identity) {  // (wave-uniform) whole frames: every row is its own image row
                    y = alive ? (orow >= a.height ? 0xFFFFFFFFu : orow) : 0u;
                    oidx = (size_t)orow * a.width + x;
                } else {
                    y = alive ? (fast_tile ? out_row_to_y_shift(a, orow) : out_row_to_y(a, orow)) : 0u;
                    oidx = (K::host_frames && !alive) ? RG_NO_PIXEL : (size_t)out_row_of(a, orow) * a.width + x;
                }
                if (K::host_frames && a.image_rows && alive)  // the whole image: the pixel's own row (padding: no store)
                    oidx = y == 0xFFFFFFFFu ? RG_NO_PIXEL : (size_t)y * a.width + x;
                if (alive && y == 0xFFFFFFFFu) {  // padding row of a partial last tile
                    if (K::host_frames && a.defer_px) *my_px = 0u;
                    else if (!K::host_frames || oidx != RG_NO_PIXEL) a.rgba[oidx] = 0u;
                    if (KDiag::rgb_is_output && out_rgb) { out_rgb[3 * oidx] = 0.0f; out_rgb[3 * oidx + 1] = 0.0f; out_rgb[3 * oidx + 2] = 0.0f; }
                    alive = false;
                }
                if constexpr (SPARSE) {  // once per tile: only the samples of flagged pixels are traced
                    if (alive) alive = a.px_mask[(size_t)(y / a.px_k) * a.px_w + x / a.px_k] != 0;
                }
                pixel = y * a.width + x;
                if (alive) {
                    RG_REGION(RGR_PRIM);
                    // ray.rs:37-54 (aspect and fov_adjustment are per-frame constants)
                    double sx, sy;
                    // heavy path: the host's per-column / per-row table of the same expressions
                    // (north star -1 %); the light path keeps the divisions (the loads at the
                    // tile's start cost it more than they save: test1 +0.5 %, test3 +1.5 %)
                    // PLAIN: neither -- the quotients from the host's reciprocals and the ray's
                    // length without range scaling, both admitted by the launcher (rg_light_plain)
                    constexpr bool fast_camera = PLAIN && RG_PLAIN_CAMERA != 0;
                    if constexpr (fast_camera) {
                        sensor_recip(a, x, y, sx, sy);
                    } else if (!K::light && a.prim_sx) {
                        sx = a.prim_sx[x];
                        sy = a.prim_sy[y];
                    } else {
                        sensor_div(a, x, y, sx, sy);
                    }
                    if constexpr (K::camera) {
                        // the launch's camera (rg_camera.h): a ray from its eye, which the loop below
                        // traces as the general closest-hit query at depth 0 that it is -- nothing of
                        // trace_primary's o = 0 (sph_cc, the planes' o.n, the camera buffer) holds for it
                        double dir[3];
                        // (the area family: with the launch's lens if it has one -- uniform across the launch;
                        // a constant for every other kernel)
                        if (K::lens || (K::area && a.lens != 0u)) {
                            // ... through the launch's thin lens (rg_lens.h): this sample's point of the lens
                            // disk, turned by the output pixel's hash, towards the plane in focus
                            double org[3];
                            rg_lens_ray(a.cam_eye, a.cam_right, a.cam_up, a.cam_forward, sx, sy, x, y, a.lens_k,
                                        a.width / a.lens_k, a.lens_focus, a.lens_r, a.lens_u,
                                        a.lens_tab + 2u * rg_lens_points_offset(a.lens_k), a.lens_tab + 2u * RG_LENS_POINTS,
                                        org, dir);
                            q.o = v3(org[0], org[1], org[2]);
                        } else {
                        rg_camera_direction(a.cam_right, a.cam_up, a.cam_forward, sx, sy, dir);
                        q.o = v3(a.cam_eye[0], a.cam_eye[1], a.cam_eye[2]);
                        }
                        q.d = v3(dir[0], dir[1], dir[2]);
                        n_prim++;
                        have_result = false;
                    } else {
                    q.o = v3(0.0, 0.0, 0.0);
                    if constexpr (fast_camera) q.d = normalize_camera(sx, sy);
                    else q.d = normalize(v3(sx, sy, -1.0));
                    n_prim++;
                    closest_init(c);
                    trace_primary<F32F, BVH, PLAIN>(a, src, q.d, c);
                    have_result = true;
                    }
                    mode = MODE_CLOSEST;
                    qdepth = 0;
                    task = -1;
                }
                if constexpr (PLAIN && RG_PLAIN_FIRST_HIT != 0) {
                    // First-hit tiles.  Every lane of the wave is here, at depth 0 with a fresh
                    // primary result or without a pixel.  A tile whose primary rays all end at a miss, a diffuse
                    // hit or a reflecting hit at the depth limit needs no frame, no mode and no parked factors:
                    // the wave shades it here in one straight line -- the general block's functions in the general
                    // block's order (rendering.rs:80-91, 141-170), so the pixels are the same bits -- and takes
                    // the next tile.  Nothing of the lane state is consumed before the wave commits: a failed
                    // vote, or a batch that could see a NaN distance, leaves the tile to the loop as it stood.
                    const bool hit = alive && c.id >= 0;
                    const int surf = hit ? T.mats[c.id].surface : RG_SURFACE_DIFFUSE;
                    const bool simple = !alive || (!c.nan && (surf == RG_SURFACE_DIFFUSE ||
                                                              (surf == RG_SURFACE_REFLECTING && 1 >= max_depth)));
                    if (!a.first_hit_off && !__any(!simple)) {  // (wave-uniform) rg_debug_set_first_hit_tiles(0): no tile
                        RG_REGION(RGR_FIRST_HIT);
                        // (the batch and its origin in the loop's own sb and q.o, which hold nothing at a tile's
                        // start: no second copy in registers.  q.o is the primary ray's origin, 0, until then.)
                        static_assert(!K::camera, "the primary rays of a PLAIN kernel leave the origin");
                        float pp[LB], lin[LB];
                        C3 bc = c3(0.0f, 0.0f, 0.0f);
                        float refl = 0.0f, rr = 0.0f;
                        [[maybe_unused]] uint32_t fw = 0u;
                        bool bail = false;
#pragma unroll
                        for (int l = 0; l < LB; ++l) pp[l] = lin[l] = 0.0f;
                        if (hit) {
                            const RgBodyDev b = T.bodies[c.id];
                            const RgMatDev m = T.mats[c.id];
                            const V3 h = add(q.o, scl(q.d, c.t));
                            V3 n;
                            if (!surface_normal(b, h, n)) bail = true;  // the general block reports it
                            const bool textured = m.coloration != RG_COLORATION_COLOR;
                            uint32_t texel = 0u;
                            if (textured) texel = texel_fetch_plain(T.texs, PT, m, b, c.id, h);
                            else bc = c3(m.color[0], m.color[1], m.color[2]);
                            refl = m.albedo_pi;      // rendering.rs:164
                            rr = m.reflectivity;     // read by a reflecting hit only (kind 1)
                            q.o = add(h, scl(n, SHADOW_BIAS));  // rendering.rs:148
                            if constexpr (SHV) {
                                fw = RG_SHVOL_ALL;
                                if (a.shvol) {  // (wave-uniform)
                                    const int cell = rg_shvol_cell((float)q.o.x, (float)q.o.y, (float)q.o.z, a.shvol_inv,
                                                                   a.shvol_off, (int)a.shvol_g);
                                    const uint32_t w = a.shvol[cell >= 0 ? cell : 0];
                                    if (cell >= 0) fw = w;
                                }
                            }
#pragma unroll
                            for (int l = 0; l < LB; ++l) {
                                const RgLightDev L = light_at<K>(a, T.lights, l, pixel);
                                light_dir_dist<UL>(L, h, sb.d[l], sb.ld[l]);
                                pp[l] = fmaxf((float)dot(n, sb.d[l]), 0.0f);  // rendering.rs:161-162
                                lin[l] = light_intensity(L, h);               // pure; used if lit
                                bail |= ray_exotic(q.o, sb.d[l]);
                            }
                            if (textured) bc = texel_color(texel);
                        }
                        if (__any(bail)) {
                            q.o = v3(0.0, 0.0, 0.0);  // the primary ray again; sb is set up anew before it is read
                        } else {  // commit: from here the tile is this path's
                            // (the primary ray and its result are spent: nothing of them lives through the walk)
                            q.d = v3(0.0, 0.0, 0.0);
                            closest_init(c);
                            uint32_t focc = 0u;
                            [[maybe_unused]] uint32_t smask = ~0u, pmask = ~0u;
                            bool walk = true;  // (wave-uniform)
                            if constexpr (SHV) {
                                if (a.shvol) {  // (a volume's scene has no body past the masks' bits: rg_shadow_vol.h)
                                    const uint32_t wm = wave_or(hit ? fw : 0u);
                                    smask = wm & 0xFFFFu;
                                    pmask = wm >> 16;
                                    walk = wm != 0u;
                                }
                            }
                            C3 fret = def;  // rendering.rs:76-77
                            if (hit) {
                                if (walk) trace_shadow<LB, PLAIN, SHV>(a, src, q.o, sb, (1u << LB) - 1u, focc, smask, pmask);
                                n_shadow += (uint32_t)LB;
                                // shade_diffuse accumulation (rendering.rs:141-170), in light order
                                C3 acc = c3(0.0f, 0.0f, 0.0f);
#pragma unroll
                                for (int l = 0; l < LB; ++l) {
                                    const RgLightDev L = light_at<K>(a, T.lights, l, pixel);
                                    const float inten = !((focc >> l) & 1u) ? lin[l] : 0.0f;
                                    const float power = pp[l] * inten;
                                    const C3 lc = cscl(cscl(c3(L.color[0], L.color[1], L.color[2]), power), refl);
                                    acc = cadd(acc, cmul(bc, lc));
                                }
                                const C3 dcol = cclamp(acc);
                                // Diffuse, or Reflecting with its ray at depth >= max (rendering.rs:86-91, 123-124)
                                fret = surf == RG_SURFACE_DIFFUSE ? dcol : cadd(cscl(dcol, 1.0f - rr), cscl(def, rr));
                            }
                            if (alive) {
                                a.rgba[oidx] = f32_to_u8(fret.r * 255.0f) | (f32_to_u8(fret.g * 255.0f) << 8) |
                                               (f32_to_u8(fret.b * 255.0f) << 16) | 0xFF000000u;
                            }
                            mode = MODE_DONE;
                            have_result = false;
                            ++n_first_hit;
                        }
                    }
                }
                continue;
            }
        }
        if constexpr (K::shadow_fan) {
            // shadow fan-out, assign: a lane about to trace the shadow ray of light li
            // hands lights li+1.. of the same hit to idle lanes of its wave, so up to
            // 1 + RG_SHADOW_FAN shadow rays of a hit are traced in one iteration instead
            // of one per iteration (the slowest pixels' ray trees are chains of such
            // iterations).  Each helper traces exactly the ray the lane would have.
            const int want = mode == MODE_SHADOW ? min(a.n_lights - li - 1, RG_SHADOW_FAN) : 0;
            unsigned long long owners = __ballot(want > 0);
            if (owners != 0ull) {
                unsigned long long idle = __ballot(mode == MODE_DONE);
                while (owners != 0ull && idle != 0ull) {
                    const int o = __builtin_ctzll(owners);
                    owners &= owners - 1ull;
                    const int w = __builtin_amdgcn_readlane(want, o);
                    const int oli = __builtin_amdgcn_readlane(li, o);
                    const int ohd = __builtin_amdgcn_readlane(hdepth, o);
                    const uint32_t opix = (uint32_t)__builtin_amdgcn_readlane((int)pixel, o);
                    const V3 ohp = v3(readlane_d(hp.x, o), readlane_d(hp.y, o), readlane_d(hp.z, o));
                    const V3 oso = v3(readlane_d(q.o.x, o), readlane_d(q.o.y, o), readlane_d(q.o.z, o));
                    uint32_t packed = 0u;
                    int k = 0;
                    for (; k < w && idle != 0ull; ++k) {
                        const int hl = __builtin_ctzll(idle);
                        idle &= idle - 1ull;
                        packed |= (uint32_t)hl << (6 * k);
                        if (lane == hl) {
                            hp = ohp;
                            q.o = oso;  // hit + n * bias (rendering.rs:148)
                            hdepth = ohd;
                            pixel = opix;  // error reports name the owner's pixel
                            light_dir_dist<UL>(light_at<K>(a, T.lights, oli + 1 + k, pixel), hp, sb.d[0], sb.ld[0]);
                            li = oli + 1 + k;  // the light this helper traces (its li is unused otherwise)
                            mode = MODE_SHADOW_H;
                        }
                    }
                    if (lane == o) {
                        nfan = k;
                        fan_lanes = packed;
                        n_shadow += (uint32_t)k;
                    }
                }
            }
        }
        if constexpr (TASKS) {
            // idle lanes take subtrees other lanes of the block published
            const bool idle = mode == MODE_DONE;
            const unsigned long long want = __ballot(idle);
            if (want != 0ull && pool_any_pending()) {
                if (idle) {
                    const int slot = pool_take((int)__builtin_amdgcn_mbcnt_hi((uint32_t)(want >> 32),
                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)want, 0u)));
                    if (slot >= 0) {
                        const double *r = pool_of().ray[slot];
                        q.o = v3(r[0], r[1], r[2]);
                        q.d = v3(r[3], r[4], r[5]);
                        qdepth = pool_of().depth[slot];
                        pixel = pool_of().pix[slot];
                        task = slot;
                        mode = MODE_CLOSEST;
                        n_sec++;  // the published reflection ray is traced here
                    }
                }
            }
        }
        const bool live = mode != MODE_DONE;
        const bool wave_live = __any(live);
        if constexpr (TASKS) {
            if (wave_live != counted) {  // the block's count of waves holding work (helpers' exit test)
                if (lane == 0) atomicAdd(&pool_of().busy, wave_live ? 1 : -1);
                counted = wave_live;
            }
        }
        if (!wave_live) {
            if (tiles_left) continue;
            if constexpr (!TASKS) break;
            // tiles exhausted: serve the block's tasks until no wave holds work
            if (!pool_any_pending() && __hip_atomic_load(&pool_of().busy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0)
                break;
            __builtin_amdgcn_s_sleep(4);
            continue;
        }
        const bool querying = mode == MODE_CLOSEST || mode == MODE_SHADOW || mode == MODE_SHADOW_H;  // WAIT lanes only poll
        if (!__any(querying)) {
            __builtin_amdgcn_s_sleep(2);
            have_result = mode == MODE_WAIT;
            continue;
        }
        KDiag::iter_stats<K::light>(a, lane, querying, mode, mode == MODE_CLOSEST ? qdepth : hdepth);
#ifdef RG_TILE_TIMES
        ++tile_iters;
        const unsigned long long t_q0 = wall_clock64();
#endif
        if (querying) {
            closest_init(c);
            occl = 0u;
        }
        if constexpr (!K::light) {
            // one ray per lane, one pass: closest-hit and shadow lanes share the
            // body loop (best when a wave mixes ray kinds over many bodies)
            if (querying) {
                bool o1 = false;
                Ray r1;
                r1.o = q.o;
                const bool shadow = mode == MODE_SHADOW || mode == MODE_SHADOW_H;
                r1.d = shadow ? sb.d[0] : q.d;
                // (a camera ray walks with its wave, as the primary ray it is, whatever lane_min_depth says)
                const bool lane_walk = (shadow ? hdepth : qdepth) >= (int)a.lane_min_depth &&
                                       !(K::camera && !shadow && qdepth == 0);
                // a shadow ray that could see a NaN distance (ray_exotic) runs as a
                // fully counted closest-hit query: in_light = none || dist > light
                // distance (rendering.rs:150-155), the scene.rs:38 panic iff >= 2 hits, one NaN
                const bool exact = shadow && (a.nan_scene || ray_exotic(r1.o, r1.d));
                // li: the light of a shadow ray (owner lanes; fan-out helpers carry the light they trace)
                trace_query<F32F, BVH>(a, src, r1, shadow && !exact, sb.ld[0], c, o1, lane_walk, shadow ? li : -1);
                if (exact) {
                    o1 = c.id >= 0 && !(c.t > sb.ld[0]);
                    if (c.nan && c.nhit >= 2) raise_error(a, pixel, RG_ERR_NAN_DISTANCE);
                }
                occl = o1 ? 1u : 0u;
            }
        } else {
            // closest-hit lanes and shadow-batch lanes walk the body tables in two
            // passes; each pass is skipped when no lane of the wave needs it.  A
            // batch that could see a NaN distance (ray_exotic) instead runs its
            // lights one by one through the closest-hit pass, fully counted
            // (rendering.rs:150-155; the scene.rs:38 panic iff >= 2 hits, one NaN).
            bool exact = false;
            if (mode == MODE_SHADOW) {
                exact = nan_scene;
#pragma unroll
                for (int l = 0; l < LB; ++l) exact |= ((occl_full >> l) & 1u) && ray_exotic(q.o, sb.d[l]);
            }
            const int passes = mode == MODE_CLOSEST ? 1 : exact ? LB : 0;
            if (exact) occl = ~occl_full & ((1u << LB) - 1u);
            for (int l = 0; __any(l < passes); ++l) {
                if (l < passes && (mode == MODE_CLOSEST || ((occl_full >> l) & 1u))) {
                    RG_REGION(RGR_Q_CLOSEST);
                    Ray rq;
                    rq.o = q.o;
                    rq.d = q.d;
                    double ld = 0.0;
                    if (exact) {
#pragma unroll
                        for (int k = 0; k < LB; ++k)
                            if (k == l) { rq.d = sb.d[k]; ld = sb.ld[k]; }
                        closest_init(c);
                    }
                    bool unused = false;
                    trace_query<F32F, BVH, PLAIN>(a, src, rq, false, 0.0, c, unused);
                    if (exact) {
                        if (c.id >= 0 && !(c.t > ld)) occl |= 1u << l;
                        if (c.nan && c.nhit >= 2) raise_error(a, pixel, RG_ERR_NAN_DISTANCE);
                    }
                }
            }
            // SHV: the wave's shadow mask -- the volume's words of the lanes about to trace a batch (each
            // set up in this iteration), ORed into one wave-uniform value (every lane is active here)
            [[maybe_unused]] uint32_t smask = ~0u, pmask = ~0u;
            if constexpr (SHV) {
                if (a.shvol) {  // (wave-uniform; spheres at bits 0..15, planes at 16..31)
                    const uint32_t wm = wave_or(mode == MODE_SHADOW && !exact ? shw : 0u);
                    smask = wm & 0xFFFFu;
                    pmask = wm >> 16;
                }
            }
            if (mode == MODE_SHADOW && !exact) {
                RG_REGION(RGR_Q_SHADOW);
                occl = ~occl_full & ((1u << LB) - 1u);  // absent slots count as done
                trace_shadow<LB, PLAIN, SHV>(a, src, q.o, sb, (1u << LB) - 1u, occl, smask, pmask);
            }
        }
#ifdef RG_TILE_TIMES
        t_query += wall_clock64() - t_q0;
#endif
        have_result = querying || mode == MODE_WAIT;
    }
    if (K::host_frames && my_tile != 0xFFFFFFFFu && (a.defer_px || a.tile_flags)) {
        bool ringed = false;
        if constexpr (RING > 0) {
            if (use_ring) {
                ring_px[rw][nring][lane] = *my_px;
                if (lane == 0) ring_tile[rw][nring] = my_tile;
                ++nring;
                ringed = true;
            }
        }
        if (!ringed) flush_tile(a, oidx, *my_px, my_tile, lane);
    }
    if constexpr (RING > 0) {
        if (use_ring) flush_ring();
    }
#ifdef RG_TILE_TIMES
    if (cur_tile != 0xFFFFFFFFu && lane == 0 && a.rgb) {  // the wave's last tile: as at a tile's start above
        a.rgb[cur_tile] = (float)(wall_clock64() - t_tile) * 0.01f;
        a.rgb[ntiles + cur_tile] = (float)tile_iters;
        a.rgb[2 * ntiles + cur_tile] = (float)(t_tile & 0xFFFFFFull);
        a.rgb[3 * ntiles + cur_tile] = (float)t_query * 0.01f;
    }
#endif

    RG_STAT(14, RG_CLOCK() - t_kernel);
    RG_STAT(15, 1);
#ifdef RG_WAVE_TIMES
    if (lane == 0 && a.rgb) {  // wave w of the grid: 4 words at rgb[4 w]
        const unsigned long long t_end = wall_clock64();
        uint32_t *wt = reinterpret_cast<uint32_t *>(a.rgb) + 4u * (blockIdx.x * (blockDim.x / 64u) + (threadIdx.x >> 6));
        wt[0] = (uint32_t)t_wave0;
        wt[1] = (uint32_t)(t_staged - t_wave0);
        wt[2] = (uint32_t)(t_end - t_wave0);
        wt[3] = wt_tiles;
    }
#endif
#ifdef RG_BVH_STATS
    if (lane >= 4 && lane < 16) atomicAdd(&a.counters[lane], rg_stat_lds[(threadIdx.x >> 6) % RG_BVH_MAX_WAVES][lane]);
#endif
    // ray counters: wave reduction, one atomic per wave per class
    unsigned long long p64 = wave_sum(n_prim), s64 = wave_sum(n_shadow), q64 = wave_sum(n_sec);
    if (lane == 0) {
        if (p64) atomicAdd(&a.counters[0], p64);
        if (s64) atomicAdd(&a.counters[1], s64);
        if (q64) atomicAdd(&a.counters[2], q64);
        if constexpr (PLAIN && RG_PLAIN_FIRST_HIT != 0) {
            if (n_first_hit) atomicAdd(&a.counters[RG_FIRST_HIT_WORD], (unsigned long long)n_first_hit);
        }
        if (a.snap_out) {
            // the last wave to finish hands the statistics words to the host itself (the copy
            // after the kernel would be a blit kernel of its own on the stream): this wave's
            // counter atomics are complete before it is counted
            __builtin_amdgcn_s_waitcnt(0);
            const unsigned long long waves = (unsigned long long)gridDim.x * (blockDim.x >> 6);
            if (atomicAdd(&a.counters[RG_DONE_WORD], 1ull) == waves - 1ull) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    a.snap_out[k] = __hip_atomic_load(&a.counters[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}
