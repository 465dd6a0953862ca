// rg_scene_tables.h — what a scene description determines, as plain host data: the tables
// rg_scene_create uploads, the scalars that go with them, and the layout of the LDS arena the
// kernels stage them into.  Built by rg_scene_build.cpp.  No HIP include: the builder and its CPU
// tests (tests/test_scene_build_cpu.py) compile with a plain C++ compiler.  Not part of the ABI.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/raingun.h"
#include "../../include/raingun_debug.h"
#include "rg_device.h"
#include "rg_lightbuf_ray.h"

// Everything rg_scene_create uploads, as host tables (kept for replicas on
// other devices: rg_render_multi).
struct rg_host_tables {
    std::vector<RgSph> sph;
    std::vector<RgSphF> sphf;
    std::vector<RgSphF2> sphf2;
    std::vector<double> sph_cc;
    std::vector<int32_t> sph_id, pln_id, dsk_id, box_id;
    std::vector<RgPln> pln;
    std::vector<RgDsk> dsk;
    std::vector<RgBox> box;
    std::vector<RgBodyDev> bodies;
    std::vector<RgMatDev> mats;
    std::vector<RgLightDev> lights;
    std::vector<RgBvhNode> nodes;
    std::vector<RgLightBufDev> lbuf;           // per light (kind RG_LB_NONE: no buffer), first RG_LB_MAX_LIGHTS lights
    std::vector<uint32_t> lb_start, lb_ent;    // every light's cell starts / list entries, concatenated
    std::vector<uint32_t> shvol;               // the shadow mask volume's words (rg_shadow_vol.h), empty: none
    std::vector<uint32_t> tex_w, tex_h;
    std::vector<std::vector<uint32_t>> texels;
    std::vector<float> amb_share;              // per body, YAML order: the ambient term's share (rg_ambient.h rg_ambient_share)
};

// The scalars the description determines: a replica shares them with its root scene, whole
// (rg_scene_replica).  Members in an order that leaves no padding, so two builds compare bytewise.
struct rg_scene_facts {
    double fov = 90.0;
    double bvh_rbound = 0.0, bvh_margin = 0.0, bvh_extent = 0.0;
    rg_bvh_info bvh_info{};
    rg_shadow_volume_info shvol_info{};  // g, bytes, build time, set share; inv / off below (rg_shvol_cell's constants)
    float shvol_inv = 0.0f, shvol_off = 0.0f;
    float bvh_obound = 0.0f;
    float def[3] = {0, 0, 0};
    int32_t n_sph = 0, n_pln = 0, n_dsk = 0, n_box = 0, n_bodies = 0, n_lights = 0, n_textures = 0;
    int32_t n_nodes = 0;     // sphere BVH (the sphere tables are in its leaf order), 0: none
    int32_t lane_stack = 0;  // per-lane walk stack entries the tree needs (0: per-lane walk unavailable)
    int32_t n_lbuf = 0;      // light slots (the first n_lbuf lights; kind NONE: no buffer)
    int32_t lb_cam = -1;     // the camera buffer's index in lbuf (primary rays), -1: none
    int32_t n_lbdesc = 0;    // descriptors in lbuf (light slots + the camera buffer)
    int32_t nan_scene = 0;   // NaN distances possible (rg_k_trace.h ray_exotic)
    int32_t pad = 0;
};
static_assert(sizeof(rg_scene_facts) == 4 * 8 + sizeof(rg_bvh_info) + sizeof(rg_shadow_volume_info) + 20 * 4, "no padding");

// The LDS arena of a launch (byte offsets, RgKernelArgs::lds_*):
// [lane stacks | sphf | sphf2 | sph | cc (padded to 16 B) | nodes | pln | dsk | box (padded) |
//  lights | texs (padded) | lbuf | bodies | mats], then, in the blob image only, the PLAIN light
// kernels' tables [texm | axes] (rg_device.h).  The hot part (staged whenever the sphere tables are)
// ends after the light-buffer descriptors: lights and texture descriptors are a few hundred bytes
// that every shadow ray / textured hit reads with a per-lane index.  The kernel stages cc, box and
// texs up to the next member's offset, hence the padding.  32-bit words only: a layout is the key
// of the image made for it (rg_lds_blob_for) and compares bytewise.
struct rg_lds_layout {
    uint32_t sphf, sph, cc, nodes, pln, dsk, box, lights, texs, lbuf, bodies, hot_bytes, mats, total_bytes;
    uint32_t texm, axes, plain_bytes;
    uint32_t n_sph, n_nodes;  // n_nodes 0: launches without the BVH
    uint32_t lbuf_staged;     // 1: the light-buffer descriptors are in the arena
};

#pragma GCC visibility push(hidden)

// Validate `d` and build every host table and fact from it: pure host arithmetic, a function of
// the description alone (only shvol_info.build_ms is a measurement).  h and f are to be freshly
// constructed.  RG_ERR_INVALID_ARGUMENT / RG_ERR_TEXTURE as rg_scene_create documents them.
rg_status rg_scene_build(const rg_scene_desc *d, rg_host_tables &h, rg_scene_facts &f);

// The arena of a launch with / without the BVH and the light buffers, behind lstack_bytes of
// per-lane walk stacks.  No allocation: it runs per launch (rg_make_args).
rg_lds_layout rg_lds_layout_of(const rg_scene_facts &f, bool bvh, bool lbuf, uint32_t lstack_bytes);

// The arena of layout L as one image of L.plain_bytes bytes, zero between the tables; texs: the
// texture descriptors as uploaded (device texel pointers).
std::vector<unsigned char> rg_lds_image(const rg_host_tables &h, const std::vector<RgTexDev> &texs, const rg_lds_layout &L);

#pragma GCC visibility pop
