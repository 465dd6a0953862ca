// rg_scene.hip — the scene behind the opaque rg_scene handle on a device: the upload of the host
// tables a description gives (built, with its validation, by rg_scene_build.cpp: no device there),
// replicas on other devices and their settings, the kernel arguments of a scene (rg_make_args:
// tables, LDS arena layout, frame constants), the arena's device image, and the scene's setters.
// No exception or abort crosses the ABI.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../../include/raingun.h"
#include "../../include/raingun_debug.h"
#include "rg_camera.h"
#include "rg_device.h"
#include "rg_area.h"
#include "rg_lens.h"
#include "rg_internal.h"

#pragma clang fp contract(off)

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

// f64::to_radians (2017 std: self * (PI / 180)), then libm tan (ray.rs:45).
double fov_adjustment(double fov) { return std::tan(fov * (3.14159265358979323846 / 180.0) / 2.0); }

void release(rg_scene *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    for (rg_frames *f : s->frames) rg_frames_detach_scene(f);
    s->frames.clear();
    rg_multi_release(s);
    rg_image_res_release(s->img);
    rg_aa_res_release(s->aa);
    rg_ambient_release(s, nullptr, true);
    // after the resource sets, whose release waits for their streams: the scene's tables and the make-once ones
    for (void *p : s->allocations) (void)hipFree(p);
    s->allocations.clear();
    if (s->lds_blob) (void)hipFree(s->lds_blob);
    s->lds_blob = nullptr;
    for (rg_launch_ctx *c : s->ctxs) rg_ctx_destroy(c);
    s->ctxs.clear();
    delete s;
}

// The host tables onto the current device, for a new scene or a replica.
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
    const rg_lds_layout L = rg_lds_layout_of(*s, bvh, a.lbuf != nullptr, a.lds_lstack_bytes);
    a.lds_sphf = L.sphf;
    a.lds_sph = L.sph;
    a.lds_cc = L.cc;
    a.lds_nodes = L.nodes;
    a.lds_pln = L.pln;
    a.lds_dsk = L.dsk;
    a.lds_box = L.box;
    a.lds_lights = L.lights;
    a.lds_texs = L.texs;
    a.lds_lbuf = L.lbuf;
    a.lds_bodies = L.bodies;
    a.lds_hot_bytes = L.hot_bytes;
    a.lds_mats = L.mats;
    a.lds_total_bytes = L.total_bytes;
    a.lds_texm = L.texm;
    a.lds_axes = L.axes;
    a.lds_plain_bytes = L.plain_bytes;
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
// made from the host tables once per arena layout; nullptr if it cannot be made.
const void *rg_lds_blob_for(const rg_scene *s, const RgKernelArgs &a) {
    const rg_lds_layout L = rg_lds_layout_of(*s, a.n_nodes > 0, a.lbuf != nullptr, a.lds_lstack_bytes);
    rg_scene *m = const_cast<rg_scene *>(s);
    if (m->lds_blob && std::memcmp(&L, &m->lds_blob_layout, sizeof L) == 0) return m->lds_blob;
    if (!s->host || L.total_bytes == 0 || L.total_bytes % 16u != 0u || L.plain_bytes % 16u != 0u) return nullptr;
    const std::vector<unsigned char> img = rg_lds_image(*s->host, s->tex_desc, L);
    void *p = nullptr;
    if (!ok(hipMalloc(&p, img.size()))) { (void)hipGetLastError(); return nullptr; }
    if (!ok(hipMemcpy(p, img.data(), img.size(), hipMemcpyHostToDevice))) { (void)hipFree(p); return nullptr; }
    if (m->lds_blob) {
        // stream-ordered launches may still read the old image: keep it with the scene's allocations
        m->allocations.push_back(m->lds_blob);
    }
    m->lds_blob = p;
    m->lds_blob_layout = L;
    return p;
}

rg_status rg_scene_replica(const rg_scene *src, int32_t device, rg_scene **out) {
    *out = nullptr;
    if (!src->host) return RG_ERR_INVALID_ARGUMENT;
    rg_scene *s = new (std::nothrow) rg_scene();
    if (!s) return RG_ERR_OUT_OF_MEMORY;
    s->device = device;
    static_cast<rg_scene_facts &>(*s) = *src;
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
    // the replica's device table follows when a frame needs it
    if (dst->light_radii != src->light_radii) dst->area_stale = true;
    static_cast<rg_scene_settings &>(*dst) = *src;
}

extern "C" {

rg_status rg_scene_create(const rg_scene_desc *d, int32_t device, rg_scene **out) {
    if (!d || !out) return RG_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if ((d->n_bodies && !d->bodies) || (d->n_lights && !d->lights) || (d->n_textures && !d->textures))
        return RG_ERR_INVALID_ARGUMENT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return RG_ERR_DEVICE;
    rg_scene *s = new (std::nothrow) rg_scene();
    if (!s) return RG_ERR_OUT_OF_MEMORY;
    std::shared_ptr<rg_host_tables> hp(new (std::nothrow) rg_host_tables());
    if (!hp) { delete s; return RG_ERR_OUT_OF_MEMORY; }
    s->device = device;
    s->max_depth = d->max_recursion_depth;
    rg_status st = rg_scene_build(d, *hp, *s);
    if (st == RG_OK && !ok(hipSetDevice(device))) st = RG_ERR_DEVICE;
    if (st == RG_OK) st = upload_tables(s, *hp);
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
