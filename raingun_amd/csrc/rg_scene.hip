// rg_scene.hip — the scene behind the opaque rg_scene handle: validation of a
// scene description, the host tables built from it (SoA hot tables + cold
// shading tables, sphere BVH, light buffers), their upload, replicas on other
// devices, and the kernel arguments of a scene (rg_make_args: tables, LDS
// arena layout, frame constants).  No exception or abort crosses the ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../../include/raingun.h"
#include "../../include/raingun_debug.h"
#include "rg_bvh.h"
#include "rg_camera.h"
#include "rg_device.h"
#include "rg_exact.h"
#include "rg_area.h"
#include "rg_lens.h"
#include "rg_lightbuf.h"
#include "rg_shadow_vol.h"
#include "rg_internal.h"

#pragma clang fp contract(off)

#ifndef RG_BVH_MIN_SPHERES
#define RG_BVH_MIN_SPHERES 16  // below this a scan of the sphere table is as cheap as a traversal
#endif

namespace {

template <class T>
rg_status upload(rg_scene *s, T **dst, const T *src, size_t n) {
    *dst = nullptr;
    if (n == 0) return RG_OK;
    void *p = nullptr;
    if (!ok(hipMalloc(&p, n * sizeof(T)))) return RG_ERR_OUT_OF_MEMORY;
    s->allocations.push_back(p);
    if (!ok(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice))) return RG_ERR_DEVICE;
    *dst = static_cast<T *>(p);
    return RG_OK;
}

double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// smallest float >= v (v finite, >= 0)
float f32_up(double v) {
    float f = (float)v;
    if ((double)f < v) f = std::nextafter(f, HUGE_VALF);
    return f;
}

// f32 pre-filter records of one sphere (bound derivation: rg_k_intersect.h, "f32 pre-filter").
void make_filter_records(const double *p, RgSphF &f, RgSphF2 &f2) {
    const double u = 5.9604644775390625e-08;  // 2^-24
    const double r2 = p[3] * p[3];            // the reference's radius * radius (bodies.rs:97)
    const double cc = dot3(p, p);
    f.cx = (float)p[0];
    f.cy = (float)p[1];
    f.cz = (float)p[2];
    f.r2hi = std::max(f32_up(r2 * (1.0 + 4.0 * u)), 1e-30f);
    f2.cchi = f32_up(cc * (1.0 + 1e-6));
    f2.cc32 = (float)cc;
    const double kd1 = u * (16.2 + 26.2 * 1.00001) * 1.01;  // primary rays: |o| = 0, |d|^2 <= 1.00001
    f2.thrp = f32_up(((double)f.r2hi + kd1 * (double)f2.cchi) * (1.0 + 1e-6));
    f2.id = -1;  // set with sph_id
}

// f64::to_radians (2017 std: self * (PI / 180)), then libm tan (ray.rs:45).
double fov_adjustment(double fov) { return std::tan(fov * (3.14159265358979323846 / 180.0) / 2.0); }

// Parameters the body tests read (bodies.rs): sphere 4, plane 6, disk 7, AABB 6.
int body_params(uint32_t kind) { return kind == RG_BODY_SPHERE ? 4 : kind == RG_BODY_DISK ? 7 : 6; }

// A body or light parameter that is non-finite or >= 1e100 in magnitude: ray
// arithmetic may then overflow to NaN distances (rg_k_trace.h ray_exotic).
bool exotic_value(double v) { return !(std::fabs(v) < 1e100); }

void release(rg_scene *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    for (rg_frames *f : s->frames) rg_frames_detach_scene(f);
    s->frames.clear();
    rg_multi_release(s);
    rg_image_res_release(s->img);
    rg_aa_res_release(s->aa);
    for (void *p : s->allocations) (void)hipFree(p);
    s->allocations.clear();
    if (s->d_ao) (void)hipFree(s->d_ao);
    s->d_ao = nullptr;
    if (s->lds_blob) (void)hipFree(s->lds_blob);
    s->lds_blob = nullptr;
    for (rg_launch_ctx *c : s->ctxs) rg_ctx_destroy(c);
    s->ctxs.clear();
    delete s;
}

// Host tables of a scene: everything rg_scene_create uploads, kept so that
// rg_render_multi can place replicas on other devices.
rg_status upload_tables(rg_scene *s, const rg_host_tables &h) {
    rg_status st = RG_OK;
#define RG_UP(dst, vec) \
    if (st == RG_OK) st = upload(s, &s->dst, h.vec.data(), h.vec.size())
    RG_UP(sph, sph);
    RG_UP(sph_cc, sph_cc);
    RG_UP(sphf, sphf);
    RG_UP(sphf2, sphf2);
    RG_UP(sph_id, sph_id);
    RG_UP(pln, pln);
    RG_UP(pln_id, pln_id);
    RG_UP(dsk, dsk);
    RG_UP(dsk_id, dsk_id);
    RG_UP(box, box);
    RG_UP(box_id, box_id);
    RG_UP(bodies, bodies);
    RG_UP(mats, mats);
    RG_UP(lights, lights);
    RG_UP(nodes, nodes);
    RG_UP(lbuf, lbuf);
    RG_UP(lb_start, lb_start);
    RG_UP(lb_ent, lb_ent);
    RG_UP(shvol, shvol);
#undef RG_UP
    // textures: RGBA8 -> one u32 per texel (one 4-byte gather per lookup)
    std::vector<RgTexDev> texs(h.tex_w.size());
    for (size_t i = 0; st == RG_OK && i < texs.size(); ++i) {
        texs[i].w = (int32_t)h.tex_w[i];
        texs[i].h = (int32_t)h.tex_h[i];
        texs[i].texels = nullptr;
        if (h.texels[i].empty()) continue;
        uint32_t *dp = nullptr;
        st = upload(s, &dp, h.texels[i].data(), h.texels[i].size());
        texs[i].texels = dp;
    }
    if (st == RG_OK) st = upload(s, &s->texs, texs.data(), texs.size());
    s->tex_desc = texs;
    return st;
}

void copy_scalars(rg_scene *dst, const rg_scene *src) {
    dst->fov = src->fov;
    std::memcpy(dst->def, src->def, sizeof dst->def);
    dst->max_depth = src->max_depth;
    dst->n_sph = src->n_sph;
    dst->n_pln = src->n_pln;
    dst->n_dsk = src->n_dsk;
    dst->n_box = src->n_box;
    dst->n_bodies = src->n_bodies;
    dst->n_lights = src->n_lights;
    dst->n_textures = src->n_textures;
    dst->n_nodes = src->n_nodes;
    dst->n_lbuf = src->n_lbuf;
    dst->lb_cam = src->lb_cam;
    dst->n_lbdesc = src->n_lbdesc;
    dst->lane_stack = src->lane_stack;
    dst->nan_scene = src->nan_scene;
    dst->bvh_obound = src->bvh_obound;
    dst->bvh_rbound = src->bvh_rbound;
    dst->bvh_margin = src->bvh_margin;
    dst->bvh_extent = src->bvh_extent;
    dst->bvh_info = src->bvh_info;
    dst->shvol_info = src->shvol_info;
    dst->shvol_inv = src->shvol_inv;
    dst->shvol_off = src->shvol_off;
}

}  // namespace

// ---------------------------------------------------------------- internal (rg_internal.h)

RgKernelArgs rg_make_args(const rg_scene *s) {
    RgKernelArgs a;
    std::memset(&a, 0, sizeof a);
    a.sph = s->sph;
    a.sph_cc = s->sph_cc;
    a.sphf = s->sphf;
    a.sphf2 = s->sphf2;
    a.path = s->path;
    a.sph_id = s->sph_id;
    a.pln = s->pln;
    a.pln_id = s->pln_id;
    a.dsk = s->dsk;
    a.dsk_id = s->dsk_id;
    a.box = s->box;
    a.box_id = s->box_id;
    a.n_sph = s->n_sph;
    a.n_pln = s->n_pln;
    a.n_dsk = s->n_dsk;
    a.n_box = s->n_box;
    const bool bvh = s->bvh_enabled && s->n_nodes > 0;
    a.nodes = bvh ? s->nodes : nullptr;
    a.n_nodes = bvh ? s->n_nodes : 0;
    a.bvh_obound = s->bvh_obound;
    a.bvh_rbound = s->bvh_rbound;
    a.bvh_margin = s->bvh_margin;
    a.bvh_extent = s->bvh_extent;
    // light buffers only with the BVH (the margins use its bounds; the kernel takes them on the BVH path)
    const bool lbuf = bvh && s->lbuf_enabled && (s->n_lbuf > 0 || s->lb_cam >= 0);
    a.lbuf = lbuf ? s->lbuf : nullptr;
    a.lb_start = lbuf ? s->lb_start : nullptr;
    a.lb_ent = lbuf ? s->lb_ent : nullptr;
    a.n_lbuf = lbuf ? s->n_lbuf : 0;
    a.lb_cam = lbuf ? s->lb_cam : -1;
    a.bodies = s->bodies;
    a.mats = s->mats;
    a.lights = s->lights;
    a.texs = s->texs;
    a.n_bodies = s->n_bodies;
    a.n_lights = s->n_lights;
    a.n_textures = s->n_textures;
    a.nan_scene = s->nan_scene ? 1 : 0;
    // per-lane BVH walk (heavy path only): stacks of lane_stack entries per thread at LDS offset 0
    const bool lane = bvh && rg_heavy_path(a) && s->lane_stack > 0 && s->lane_min_depth < 1 << 20;
    a.lane_stack = lane ? s->lane_stack : 0;
    a.lane_min_depth = lane ? s->lane_min_depth : 1 << 30;
    // lane_stack entries + one spare slot per lane (rg_k_bvh.h bvh_lane, RG_LANE_BRANCHFREE)
    a.lds_lstack_bytes = lane ? ((uint32_t)(a.lane_stack + 1) * 4u) * 256u * RG_HEAVY_WPS : 0u;
    // LDS arena: [lane stacks | sphf | sphf2 | sph | cc (padded to 16 B) | nodes | pln | dsk | box (padded) |
    //             lights | texs (padded) | bodies | mats].  The hot part (staged whenever the sphere
    //             tables are) ends after the texture descriptors: lights and texture descriptors are a
    //             few hundred bytes that every shadow ray / textured hit reads with a per-lane index.
    auto al16 = [](uint32_t v) { return (v + 15u) & ~15u; };
    a.lds_sphf = a.lds_lstack_bytes;
    a.lds_sph = a.lds_sphf + (uint32_t)s->n_sph * (uint32_t)(sizeof(RgSphF) + sizeof(RgSphF2));
    a.lds_cc = a.lds_sph + (uint32_t)s->n_sph * (uint32_t)sizeof(RgSph);
    a.lds_nodes = al16(a.lds_cc + (uint32_t)s->n_sph * 8u);
    a.lds_pln = a.lds_nodes + (uint32_t)a.n_nodes * (uint32_t)sizeof(RgBvhNode);
    a.lds_dsk = a.lds_pln + (uint32_t)s->n_pln * (uint32_t)sizeof(RgPln);
    a.lds_box = a.lds_dsk + (uint32_t)s->n_dsk * (uint32_t)sizeof(RgDsk);
    a.lds_lights = al16(a.lds_box + (uint32_t)s->n_box * (uint32_t)sizeof(RgBox));
    a.lds_texs = a.lds_lights + (uint32_t)s->n_lights * (uint32_t)sizeof(RgLightDev);
    a.lds_lbuf = al16(a.lds_texs + (uint32_t)s->n_textures * (uint32_t)sizeof(RgTexDev));
    a.lds_bodies = a.lds_lbuf + (a.lbuf ? (uint32_t)s->n_lbdesc * (uint32_t)sizeof(RgLightBufDev) : 0u);
    a.lds_hot_bytes = a.lds_bodies;
    a.lds_mats = a.lds_bodies + (uint32_t)s->n_bodies * (uint32_t)sizeof(RgBodyDev);
    a.lds_total_bytes = a.lds_mats + (uint32_t)s->n_bodies * (uint32_t)sizeof(RgMatDev);
    // behind the arena, in the blob image only: the PLAIN light kernels' tables (rg_device.h)
    a.lds_texm = a.lds_total_bytes;
    a.lds_axes = a.lds_texm + (uint32_t)s->n_textures * (uint32_t)sizeof(RgTexMagic);
    a.lds_plain_bytes = a.lds_axes + (uint32_t)s->n_bodies * (uint32_t)sizeof(RgPlnAxes);
    a.def[0] = s->def[0];
    a.def[1] = s->def[1];
    a.def[2] = s->def[2];
    a.max_depth = s->max_depth;
    a.fov_adjustment = fov_adjustment(s->fov);
    a.tile_wlog = 3;  // 8x8 tiles
    // the shadow mask volume (PLAIN light kernels; rg_debug_set_shadow_volume(0): none)
    const bool shvol = RG_PLAIN_SHVOL != 0 && s->shvol_enabled && s->shvol != nullptr;
    a.shvol = shvol ? s->shvol : nullptr;
    a.shvol_g = shvol ? (uint32_t)s->shvol_info.g : 0u;
    a.shvol_inv = s->shvol_inv;
    a.shvol_off = s->shvol_off;
    a.first_hit_off = s->first_hit_enabled ? 0u : 1u;  // rg_debug_set_first_hit_tiles(0)
    return a;
}

double rg_fov_adjustment(double fov) { return fov_adjustment(fov); }

bool rg_scene_heavy(const rg_scene *s) {
    RgKernelArgs a;  // only what rg_heavy_path reads
    std::memset(&a, 0, sizeof a);
    a.n_sph = s->n_sph;
    a.n_pln = s->n_pln;
    a.n_dsk = s->n_dsk;
    a.n_box = s->n_box;
    a.path = s->path;
    a.n_lights = s->n_lights;
    return rg_heavy_path(a);
}

// The LDS arena of launch args `a` as one device image (light path: RgKernelArgs::lds_blob),
// built from the host tables once per arena layout; nullptr if it cannot be made.
const void *rg_lds_blob_for(const rg_scene *s, const RgKernelArgs &a) {
    const uint32_t layout[14] = {a.lds_sphf, a.lds_sph, a.lds_cc, a.lds_nodes, a.lds_pln, a.lds_dsk, a.lds_box,
                                 a.lds_bodies, a.lds_mats, a.lds_lights, a.lds_texs, a.lds_total_bytes,
                                 (uint32_t)a.n_nodes, (uint32_t)a.n_sph};
    rg_scene *m = const_cast<rg_scene *>(s);
    if (m->lds_blob && std::memcmp(layout, m->lds_blob_layout, sizeof layout) == 0) return m->lds_blob;
    if (!s->host || a.lds_total_bytes == 0 || a.lds_total_bytes % 16u != 0u || a.lds_plain_bytes % 16u != 0u)
        return nullptr;
    const rg_host_tables &h = *s->host;
    std::vector<unsigned char> img(a.lds_plain_bytes, 0);
    auto put = [&](uint32_t off, const void *src, size_t bytes) {
        if (bytes && off + bytes <= img.size()) std::memcpy(img.data() + off, src, bytes);
    };
    put(a.lds_sphf, h.sphf.data(), h.sphf.size() * sizeof(RgSphF));
    put(a.lds_sphf + (uint32_t)(h.sphf.size() * sizeof(RgSphF)), h.sphf2.data(), h.sphf2.size() * sizeof(RgSphF2));
    put(a.lds_sph, h.sph.data(), h.sph.size() * sizeof(RgSph));
    put(a.lds_cc, h.sph_cc.data(), h.sph_cc.size() * sizeof(double));
    if (a.n_nodes > 0) put(a.lds_nodes, h.nodes.data(), h.nodes.size() * sizeof(RgBvhNode));
    put(a.lds_pln, h.pln.data(), h.pln.size() * sizeof(RgPln));
    put(a.lds_dsk, h.dsk.data(), h.dsk.size() * sizeof(RgDsk));
    put(a.lds_box, h.box.data(), h.box.size() * sizeof(RgBox));
    put(a.lds_bodies, h.bodies.data(), h.bodies.size() * sizeof(RgBodyDev));
    put(a.lds_mats, h.mats.data(), h.mats.size() * sizeof(RgMatDev));
    put(a.lds_lights, h.lights.data(), h.lights.size() * sizeof(RgLightDev));
    put(a.lds_texs, s->tex_desc.data(), s->tex_desc.size() * sizeof(RgTexDev));
    if (a.lbuf) put(a.lds_lbuf, h.lbuf.data(), h.lbuf.size() * sizeof(RgLightBufDev));
    // the PLAIN light kernels' tables: each texture dimension's magic, each plane's texture axes
    std::vector<RgTexMagic> texm(h.tex_w.size(), RgTexMagic{0, 0, 0, 0});
    for (size_t t = 0; t < texm.size(); ++t) {
        if (h.tex_w[t] == 0 || h.tex_h[t] == 0) continue;
        const RgMagicU32 mw = rg_magic_u32(h.tex_w[t]), mh = rg_magic_u32(h.tex_h[t]);
        texm[t] = RgTexMagic{mw.m, mw.sh, mh.m, mh.sh};
    }
    put(a.lds_texm, texm.data(), texm.size() * sizeof(RgTexMagic));
    std::vector<RgPlnAxes> axes(h.bodies.size());
    std::memset(axes.data(), 0, axes.size() * sizeof(RgPlnAxes));
    for (size_t b = 0; b < axes.size(); ++b)
        if (h.bodies[b].kind == RG_BODY_PLANE) rg_plane_axes(&h.bodies[b].p[3], axes[b].xa, axes[b].ya);
    put(a.lds_axes, axes.data(), axes.size() * sizeof(RgPlnAxes));
    void *p = nullptr;
    if (!ok(hipMalloc(&p, img.size()))) { (void)hipGetLastError(); return nullptr; }
    if (!ok(hipMemcpy(p, img.data(), img.size(), hipMemcpyHostToDevice))) { (void)hipFree(p); return nullptr; }
    if (m->lds_blob) {
        // stream-ordered launches may still read the old image: keep it with the scene's allocations
        m->allocations.push_back(m->lds_blob);
    }
    m->lds_blob = p;
    std::memcpy(m->lds_blob_layout, layout, sizeof layout);
    return p;
}

rg_status rg_scene_replica(const rg_scene *src, int32_t device, rg_scene **out) {
    *out = nullptr;
    if (!src->host) return RG_ERR_INVALID_ARGUMENT;
    rg_scene *s = new (std::nothrow) rg_scene();
    if (!s) return RG_ERR_OUT_OF_MEMORY;
    s->device = device;
    copy_scalars(s, src);
    rg_sync_settings(s, src);
    s->host = src->host;
    if (!ok(hipSetDevice(device))) { release(s); return RG_ERR_DEVICE; }
    rg_status st = upload_tables(s, *src->host);
    if (st == RG_OK && !(s->last = rg_ctx_for(s, nullptr))) st = RG_ERR_OUT_OF_MEMORY;
    if (st != RG_OK) { release(s); return st; }
    *out = s;
    return RG_OK;
}

void rg_scene_free(rg_scene *s) { release(s); }

rg_status rg_area_upload(rg_scene *s) {
    const uint32_t n = rg_area_table_doubles((uint32_t)s->n_lights);
    std::vector<double> table(n, 0.0);
    rg_area_make_table_points(table.data());
    for (size_t l = 0; l < s->light_radii.size() && l < (size_t)s->n_lights; ++l) table[RG_AREA_POINT_DOUBLES + l] = s->light_radii[l];
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    if (!s->d_area) {
        void *p = nullptr;
        if (!ok(hipMalloc(&p, n * sizeof(double)))) {
            (void)hipGetLastError();
            return RG_ERR_OUT_OF_MEMORY;
        }
        s->allocations.push_back(p);
        s->d_area = static_cast<double *>(p);
    }
    // launches enqueued earlier read the table by reference: let them finish, then rewrite it
    if (!ok(hipDeviceSynchronize()) || !ok(hipMemcpy(s->d_area, table.data(), n * sizeof(double), hipMemcpyHostToDevice)))
        return RG_ERR_DEVICE;
    s->area_stale = false;
    return RG_OK;
}

void rg_sync_settings(rg_scene *dst, const rg_scene *src) {
    dst->max_depth = src->max_depth;
    dst->path = src->path;
    dst->bvh_enabled = src->bvh_enabled;
    dst->lbuf_enabled = src->lbuf_enabled;
    dst->shvol_enabled = src->shvol_enabled;
    dst->first_hit_enabled = src->first_hit_enabled;
    dst->exact_div = src->exact_div;
    dst->has_camera = src->has_camera;
    dst->camera = src->camera;
    dst->lens = src->lens;
    if (dst->light_radii != src->light_radii) {  // the replica's device table follows when a frame needs it
        dst->light_radii = src->light_radii;
        dst->area_stale = true;
    }
    dst->area_any = src->area_any;
    dst->lane_min_depth = src->lane_min_depth;
    dst->tile_order = src->tile_order;
    dst->ring_flush_small = src->ring_flush_small;
    dst->ring_group_small = src->ring_group_small;
    dst->ring_flush_big = src->ring_flush_big;
    dst->ring_group_big = src->ring_group_big;
}

extern "C" {

rg_status rg_scene_create(const rg_scene_desc *d, int32_t device, rg_scene **out) {
    if (!d || !out) return RG_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if ((d->n_bodies && !d->bodies) || (d->n_lights && !d->lights) || (d->n_textures && !d->textures))
        return RG_ERR_INVALID_ARGUMENT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return RG_ERR_DEVICE;
    // validate enums and textures on the host first
    bool nan_scene = false;
    for (uint32_t i = 0; i < d->n_bodies; ++i) {
        const rg_body &b = d->bodies[i];
        if (b.kind > RG_BODY_AABB || b.material.coloration > RG_COLORATION_TEXTURE ||
            b.material.surface > RG_SURFACE_REFRACTIVE)
            return RG_ERR_INVALID_ARGUMENT;
        if (b.material.coloration == RG_COLORATION_TEXTURE) {
            int32_t t = b.material.texture;
            if (t < 0 || (uint32_t)t >= d->n_textures || !d->textures[t].rgba || d->textures[t].width == 0 ||
                d->textures[t].height == 0 || d->textures[t].width > 0x7fffffffu || d->textures[t].height > 0x7fffffffu)
                return RG_ERR_TEXTURE;
        }
        for (int k = 0; k < body_params(b.kind); ++k) nan_scene |= exotic_value(b.p[k]);
    }
    for (uint32_t i = 0; i < d->n_lights; ++i) {
        if (d->lights[i].kind > RG_LIGHT_SPHERICAL) return RG_ERR_INVALID_ARGUMENT;
        for (int k = 0; k < 3; ++k) nan_scene |= exotic_value(d->lights[i].v[k]);
    }

    rg_scene *s = new (std::nothrow) rg_scene();
    if (!s) return RG_ERR_OUT_OF_MEMORY;
    std::shared_ptr<rg_host_tables> hp(new (std::nothrow) rg_host_tables());
    if (!hp) { delete s; return RG_ERR_OUT_OF_MEMORY; }
    rg_host_tables &h = *hp;
    s->device = device;
    s->fov = d->fov;
    std::memcpy(s->def, d->default_color, sizeof s->def);
    s->max_depth = d->max_recursion_depth;
    s->nan_scene = nan_scene;
    if (!ok(hipSetDevice(device))) { release(s); return RG_ERR_DEVICE; }

    std::vector<double> sph_raw;  // center xyz, radius (BVH build input)
    h.bodies.resize(d->n_bodies);
    h.mats.resize(d->n_bodies);
    for (uint32_t i = 0; i < d->n_bodies; ++i) {
        const rg_body &b = d->bodies[i];
        const double *p = b.p;
        h.bodies[i].kind = (int32_t)b.kind;
        h.bodies[i].pad = 0;
        std::memcpy(h.bodies[i].p, b.p, sizeof h.bodies[i].p);
        const rg_material &m = b.material;
        RgMatDev &md = h.mats[i];
        md.coloration = (int32_t)m.coloration;
        std::memcpy(md.color, m.color, sizeof md.color);
        md.tex = m.texture;
        md.xoff = m.x_offset;
        md.yoff = m.y_offset;
        md.albedo_pi = m.albedo / 3.14159265358979323846f;  // std::f32::consts::PI, IEEE f32 division
        md.surface = (int32_t)m.surface;
        md.reflectivity = m.reflectivity;
        md.index = m.index;
        md.transparency = m.transparency;
        switch (b.kind) {
        case RG_BODY_SPHERE:
            // r2 = radius * radius and cc = (c.c) evaluated exactly as the per-ray
            // reference expressions (bodies.rs:95,97) -> bit-identical.
            h.sph.push_back(RgSph{p[0], p[1], p[2], p[3] * p[3]});
            h.sphf.emplace_back();
            h.sphf2.emplace_back();
            make_filter_records(p, h.sphf.back(), h.sphf2.back());
            h.sphf2.back().id = (int32_t)i;  // the record a leaf test already holds carries the id
            h.sph_cc.push_back(dot3(p, p));  // padded to an even count after the loop
            h.sph_id.push_back((int32_t)i);
            sph_raw.insert(sph_raw.end(), p, p + 4);
            break;
        case RG_BODY_PLANE:
            h.pln.push_back(RgPln{p[0], p[1], p[2], p[3], p[4], p[5], dot3(p, p + 3), 0.0});
            h.pln_id.push_back((int32_t)i);
            break;
        case RG_BODY_DISK:
            h.dsk.push_back(RgDsk{p[0], p[1], p[2], p[3], p[4], p[5], p[6], dot3(p, p + 3)});
            h.dsk_id.push_back((int32_t)i);
            break;
        default:
            h.box.push_back(RgBox{{p[0], p[1], p[2]}, {p[3], p[4], p[5]}});
            h.box_id.push_back((int32_t)i);
            break;
        }
    }
    // Sphere BVH: reorder the sphere tables into leaf order (sph_id keeps the
    // YAML index, so the closest-hit tie-break is unaffected).  Not for scenes
    // whose arithmetic may produce NaN distances: the scene.rs:38 panic needs
    // every ray's hit count, which a pruned traversal does not see.
    RgBvhBuild bvh;
    if (!nan_scene && (int)h.sph.size() >= RG_BVH_MIN_SPHERES && rg_build_bvh(sph_raw.data(), (int)h.sph.size(), bvh)) {
        auto permute = [&](auto &v) {
            auto old = v;
            for (size_t j = 0; j < bvh.order.size(); ++j) v[j] = old[bvh.order[j]];
        };
        permute(h.sph);
        permute(h.sphf);
        permute(h.sphf2);
        permute(h.sph_cc);
        permute(h.sph_id);
        s->bvh_obound = bvh.obound;
        s->bvh_rbound = bvh.rbound;
        s->bvh_margin = bvh.margin;
        s->bvh_extent = bvh.extent;
        s->bvh_info.built = 1;
        s->bvh_info.nodes = (int32_t)bvh.nodes.size();
        s->bvh_info.leaves = bvh.leaves;
        s->bvh_info.depth = bvh.depth;
        s->bvh_info.lane_stack = bvh.lane_stack;
        s->bvh_info.margin = (float)bvh.margin;
        s->bvh_info.origin_bound = bvh.obound;
        h.nodes = bvh.nodes;
    }
    if (h.sph_cc.size() % 2) h.sph_cc.push_back(0.0);  // LDS staging copies 16-B units
    h.lights.resize(d->n_lights);
    for (uint32_t i = 0; i < d->n_lights; ++i) {
        const rg_light &l = d->lights[i];
        RgLightDev &ld = h.lights[i];
        ld.kind = (int32_t)l.kind;
        std::memcpy(ld.color, l.color, sizeof ld.color);
        ld.intensity = l.intensity;
        ld.pad = 0;
        std::memcpy(ld.v, l.v, sizeof ld.v);
        // Directional: normalize(-direction) (lights.rs:48) is a per-light constant.
        // Same IEEE ops in the same order as the device would run -> identical bits.
        double nx = -l.v[0], ny = -l.v[1], nz = -l.v[2];
        double inv = 1.0 / std::sqrt((nx * nx + ny * ny) + nz * nz);
        ld.dn[0] = nx * inv;
        ld.dn[1] = ny * inv;
        ld.dn[2] = nz * inv;
        ld.pad2 = 0.0;
    }
    // Shadow-ray light buffers (rg_lightbuf.cpp) over the BVH-ordered sphere tables, for the first
    // RG_LB_MAX_LIGHTS lights; a light that cannot be served well keeps the BVH walk (kind NONE)
    if (!h.nodes.empty()) {
        std::vector<double> sp(4 * h.sph.size());
        for (size_t j = 0; j < h.sph.size(); ++j) {
            const double *p = &sph_raw[4 * (size_t)bvh.order[j]];  // centre, radius of BVH position j
            std::memcpy(&sp[4 * j], p, 4 * sizeof(double));
        }
        const uint32_t nl = std::min<uint32_t>(d->n_lights, RG_LB_MAX_LIGHTS);
        h.lbuf.assign(nl, RgLightBufDev{});
        int built = 0;
        for (uint32_t i = 0; i < nl; ++i) {
            RgLightBufBuild lb;
            if (!rg_build_lightbuf(sp.data(), (int)h.sph.size(), h.lights[i].kind, h.lights[i].dn, h.lights[i].v,
                                   bvh.extent, (double)bvh.obound, lb))
                continue;
            // a budget on all buffers together: past it, a light keeps the BVH walk
            if (h.lb_ent.size() + lb.ent.size() + h.lb_start.size() + lb.start.size() > RG_LB_TOTAL_WORDS) continue;
            const uint32_t ebase = (uint32_t)h.lb_ent.size(), cbase = (uint32_t)h.lb_start.size();
            for (uint32_t &v : lb.start) v += ebase;
            lb.dev.cell_off = cbase;
            lb.dev.always0 += ebase;
            lb.dev.always1 += ebase;
            h.lb_start.insert(h.lb_start.end(), lb.start.begin(), lb.start.end());
            h.lb_ent.insert(h.lb_ent.end(), lb.ent.begin(), lb.ent.end());
            h.lbuf[i] = lb.dev;
            ++built;
        }
        // the camera buffer: a light buffer around the camera (ray.rs:53: every primary ray starts at
        // the origin), behind the lights' slots; primary rays test their direction's cell
        const double zero[3] = {0.0, 0.0, 0.0};
        RgLightBufBuild cam;
        if (rg_build_lightbuf(sp.data(), (int)h.sph.size(), RG_LIGHT_SPHERICAL, zero, zero, bvh.extent,
                              (double)bvh.obound, cam) &&
            h.lb_ent.size() + cam.ent.size() + h.lb_start.size() + cam.start.size() <= RG_LB_TOTAL_WORDS) {
            const uint32_t ebase = (uint32_t)h.lb_ent.size(), cbase = (uint32_t)h.lb_start.size();
            for (uint32_t &v : cam.start) v += ebase;
            cam.dev.cell_off = cbase;
            cam.dev.always0 += ebase;
            cam.dev.always1 += ebase;
            h.lb_start.insert(h.lb_start.end(), cam.start.begin(), cam.start.end());
            h.lb_ent.insert(h.lb_ent.end(), cam.ent.begin(), cam.ent.end());
            s->lb_cam = (int32_t)h.lbuf.size();
            h.lbuf.push_back(cam.dev);
        }
        if (!built && s->lb_cam < 0) h.lbuf.clear();
        s->n_lbuf = built ? (int32_t)nl : 0;
        s->n_lbdesc = (int32_t)h.lbuf.size();
        s->bvh_info.lbuf_bytes = (int64_t)((h.lb_ent.size() + h.lb_start.size()) * sizeof(uint32_t) +
                                           h.lbuf.size() * sizeof(RgLightBufDev));
    }
    // Shadow mask volume (rg_shadow_vol.cpp) over the sphere and plane tables in kernel order: scenes
    // the PLAIN light kernels can run (no disks, no boxes)
    if (RG_PLAIN_SHVOL != 0 && h.dsk.empty() && h.box.empty() && !nan_scene) {
        std::vector<double> sp(sph_raw);  // centre, radius by table position (a BVH reorders the tables)
        for (size_t j = 0; !h.nodes.empty() && j < h.sph.size(); ++j)
            std::memcpy(&sp[4 * j], &sph_raw[4 * (size_t)bvh.order[j]], 4 * sizeof(double));
        std::vector<double> pl(6 * h.pln.size());
        for (size_t j = 0; j < h.pln.size(); ++j) {
            const RgPln &p = h.pln[j];
            const double v[6] = {p.ox, p.oy, p.oz, p.nx, p.ny, p.nz};
            std::memcpy(&pl[6 * j], v, sizeof v);
        }
        std::vector<RgShadowVolLight> ls(h.lights.size());
        for (size_t l = 0; l < ls.size(); ++l) {
            ls[l].kind = h.lights[l].kind;
            std::memcpy(ls[l].v, h.lights[l].v, sizeof ls[l].v);
            std::memcpy(ls[l].dn, h.lights[l].dn, sizeof ls[l].dn);
        }
        RgShadowVolBuild sv;
        if (rg_build_shadow_vol(sp.data(), (int)h.sph.size(), pl.data(), (int)h.pln.size(), ls.data(), (int)ls.size(),
                                RG_SHVOL_G, sv)) {
            s->shvol_info.built = 1;
            s->shvol_info.g = sv.g;
            s->shvol_info.bytes = (int64_t)(sv.words.size() * sizeof(uint32_t));
            s->shvol_info.build_ms = sv.build_ms;
            s->shvol_info.set_share = sv.set_share;
            s->shvol_inv = sv.inv;
            s->shvol_off = sv.off;
            h.shvol = std::move(sv.words);
        }
    }
    h.tex_w.resize(d->n_textures);
    h.tex_h.resize(d->n_textures);
    h.texels.resize(d->n_textures);
    for (uint32_t i = 0; i < d->n_textures; ++i) {
        const rg_texture &t = d->textures[i];
        h.tex_w[i] = t.width;
        h.tex_h[i] = t.height;
        const size_t n = (size_t)t.width * t.height;
        if (n == 0 || !t.rgba) continue;
        h.texels[i].resize(n);
        std::memcpy(h.texels[i].data(), t.rgba, n * 4);
    }
    s->n_sph = (int32_t)h.sph.size();
    s->n_pln = (int32_t)h.pln.size();
    s->n_dsk = (int32_t)h.dsk.size();
    s->n_box = (int32_t)h.box.size();
    s->n_bodies = (int32_t)d->n_bodies;
    s->n_lights = (int32_t)d->n_lights;
    s->n_textures = (int32_t)d->n_textures;
    s->n_nodes = (int32_t)h.nodes.size();
    // the stack entry keeps the node index in its low RG_LANE_NODE_BITS bits
    s->lane_stack = (s->n_nodes <= (1 << RG_LANE_NODE_BITS) && bvh.lane_stack <= RG_LANE_STACK_MAX)
                        ? std::max(bvh.lane_stack, 1) : 0;

    rg_status st = upload_tables(s, h);
    s->host = hp;
    if (st == RG_OK && !(s->last = rg_ctx_for(s, nullptr))) st = RG_ERR_OUT_OF_MEMORY;  // default-stream context
    if (st != RG_OK) { release(s); return st; }
    *out = s;
    return RG_OK;
}

void rg_scene_destroy(rg_scene *s) { release(s); }

rg_status rg_scene_set_max_depth(rg_scene *s, uint32_t max_depth) {
    if (!s) return RG_ERR_INVALID_ARGUMENT;
    s->max_depth = max_depth;
    return RG_OK;
}

rg_status rg_camera_look_at(const double eye[3], const double target[3], const double up[3], rg_camera *out) {
    if (!eye || !target || !up || !out) return RG_ERR_INVALID_ARGUMENT;
    rg_camera c;
    if (!rg_camera_look_at_basis(eye, target, up, c.right, c.up, c.forward)) return RG_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < 3; ++k) c.eye[k] = eye[k];
    *out = c;
    return RG_OK;
}

rg_status rg_scene_set_camera(rg_scene *s, const rg_camera *camera) {
    if (!s) return RG_ERR_INVALID_ARGUMENT;
    if (!camera) {  // the reference's view again: the launches and kernels of a scene that never had a camera
        s->has_camera = false;
        return RG_OK;
    }
    if (!rg_camera_valid(camera->eye, camera->right, camera->up, camera->forward)) return RG_ERR_INVALID_ARGUMENT;
    s->camera = *camera;
    s->has_camera = true;
    return RG_OK;
}

rg_status rg_scene_set_lens(rg_scene *s, const rg_lens *lens) {
    if (!s) return RG_ERR_INVALID_ARGUMENT;
    if (!lens) {  // the pinhole again: the launches and kernels of a scene that never had a lens
        s->lens = rg_lens{0.0, 1.0};
        return RG_OK;
    }
    if (!rg_lens_valid(lens->aperture, lens->focus)) return RG_ERR_INVALID_ARGUMENT;
    s->lens = *lens;
    return RG_OK;
}

rg_status rg_scene_set_light_radii(rg_scene *s, const double *radii, uint32_t n) {
    if (!s) return RG_ERR_INVALID_ARGUMENT;
    if (!radii) {  // point lights again: the launches and kernels of a scene that never had radii
        s->light_radii.clear();
        s->area_any = false;
        return RG_OK;
    }
    if (n != (uint32_t)s->n_lights || !s->host) return RG_ERR_INVALID_ARGUMENT;
    bool any = false;
    for (uint32_t l = 0; l < n; ++l) {
        if (!rg_area_radius_valid(radii[l])) return RG_ERR_INVALID_ARGUMENT;
        // a directional light has no position to spread
        if (radii[l] > 0.0 && s->host->lights[l].kind == RG_LIGHT_DIRECTIONAL) return RG_ERR_INVALID_ARGUMENT;
        any |= radii[l] > 0.0;
    }
    const std::vector<double> kept = s->light_radii;
    s->light_radii.assign(radii, radii + n);
    if (any) {  // only frames with a radius > 0 read the table
        const rg_status st = rg_area_upload(s);
        if (st != RG_OK) {
            s->light_radii = kept;
            return st;
        }
    }
    s->area_any = any;
    return RG_OK;
}

rg_status rg_area_tables(uint32_t samples, double *points) {
    if (samples < 1 || samples > RG_LENS_MAX_SAMPLES || !points) return RG_ERR_INVALID_ARGUMENT;
    rg_area_make_points(samples, points);
    return RG_OK;
}

rg_status rg_lens_tables(uint32_t samples, double *points, double *rotations) {
    if (samples < 1 || samples > RG_LENS_MAX_SAMPLES || !points) return RG_ERR_INVALID_ARGUMENT;
    rg_lens_make_points(samples, points);
    if (rotations) rg_lens_make_rotations(rotations);
    return RG_OK;
}

}  // extern "C"
