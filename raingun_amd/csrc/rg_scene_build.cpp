// rg_scene_build.cpp — a scene description into host tables (rg_scene_tables.h): validation, the
// SoA hot tables and cold shading tables, the f32 filter records, the sphere BVH and its reorder,
// the light buffers, the shadow mask volume, the textures; and the LDS arena's layout and image.
// Plain host C++, a function of the description alone: it runs, and is tested, without a device
// (tests/test_scene_build_cpu.py).  Its f64/f32 arithmetic states the reference's, operation by
// operation; the library is built unfused (-ffp-contract=off).
#if defined(__HIP__)
#include <hip/hip_runtime.h>  // hipcc builds this file as HIP (host code only)
#endif
#include "rg_scene_tables.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "rg_ambient.h"
#include "rg_bvh.h"
#include "rg_exact.h"
#include "rg_lightbuf.h"
#include "rg_shadow_vol.h"

#ifndef RG_BVH_MIN_SPHERES
#define RG_BVH_MIN_SPHERES 16  // below this a scan of the sphere table is as cheap as a traversal
#endif

namespace {

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

// Parameters the body tests read (bodies.rs): sphere 4, plane 6, disk 7, AABB 6.
int body_params(uint32_t kind) { return kind == RG_BODY_SPHERE ? 4 : kind == RG_BODY_DISK ? 7 : 6; }

// A body or light parameter that is non-finite or >= 1e100 in magnitude: ray
// arithmetic may then overflow to NaN distances (rg_k_trace.h ray_exotic).
bool exotic_value(double v) { return !(std::fabs(v) < 1e100); }

// Enums, array pointers and textures of a description; *nan_scene: a parameter is exotic.
rg_status validate(const rg_scene_desc *d, bool *nan_scene) {
    if (!d || (d->n_bodies && !d->bodies) || (d->n_lights && !d->lights) || (d->n_textures && !d->textures))
        return RG_ERR_INVALID_ARGUMENT;
    *nan_scene = false;
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
        for (int k = 0; k < body_params(b.kind); ++k) *nan_scene |= exotic_value(b.p[k]);
    }
    for (uint32_t i = 0; i < d->n_lights; ++i) {
        if (d->lights[i].kind > RG_LIGHT_SPHERICAL) return RG_ERR_INVALID_ARGUMENT;
        for (int k = 0; k < 3; ++k) *nan_scene |= exotic_value(d->lights[i].v[k]);
    }
    return RG_OK;
}

// Append one light buffer's cell starts and entries to the scene's, its offsets rebased onto them;
// false (nothing appended) past the budget on all buffers together: the light keeps the BVH walk.
bool append_lightbuf(rg_host_tables &h, RgLightBufBuild &lb) {
    if (h.lb_ent.size() + lb.ent.size() + h.lb_start.size() + lb.start.size() > RG_LB_TOTAL_WORDS) return false;
    const uint32_t ebase = (uint32_t)h.lb_ent.size(), cbase = (uint32_t)h.lb_start.size();
    for (uint32_t &v : lb.start) v += ebase;
    lb.dev.cell_off = cbase;
    lb.dev.always0 += ebase;
    lb.dev.always1 += ebase;
    h.lb_start.insert(h.lb_start.end(), lb.start.begin(), lb.start.end());
    h.lb_ent.insert(h.lb_ent.end(), lb.ent.begin(), lb.ent.end());
    return true;
}

}  // namespace

rg_status rg_scene_build(const rg_scene_desc *d, rg_host_tables &h, rg_scene_facts &f) {
    bool nan_scene = false;
    const rg_status vst = validate(d, &nan_scene);
    if (vst != RG_OK) return vst;
    f.fov = d->fov;
    std::memcpy(f.def, d->default_color, sizeof f.def);
    f.nan_scene = nan_scene ? 1 : 0;

    std::vector<double> sp;  // centre xyz, radius by sphere-table position (the builders' input)
    h.bodies.resize(d->n_bodies);
    h.mats.resize(d->n_bodies);
    h.amb_share.resize(d->n_bodies);
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
        h.amb_share[i] = rg_ambient_share(m.surface, m.albedo, m.reflectivity);
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
            sp.insert(sp.end(), p, p + 4);
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
    if (!nan_scene && (int)h.sph.size() >= RG_BVH_MIN_SPHERES && rg_build_bvh(sp.data(), (int)h.sph.size(), bvh)) {
        auto permute = [&](auto &v) {
            auto old = v;
            for (size_t j = 0; j < bvh.order.size(); ++j) v[j] = old[bvh.order[j]];
        };
        permute(h.sph);
        permute(h.sphf);
        permute(h.sphf2);
        permute(h.sph_cc);
        permute(h.sph_id);
        const std::vector<double> raw = sp;
        for (size_t j = 0; j < bvh.order.size(); ++j)
            std::memcpy(&sp[4 * j], &raw[4 * (size_t)bvh.order[j]], 4 * sizeof(double));
        f.bvh_obound = bvh.obound;
        f.bvh_rbound = bvh.rbound;
        f.bvh_margin = bvh.margin;
        f.bvh_extent = bvh.extent;
        f.bvh_info.built = 1;
        f.bvh_info.nodes = (int32_t)bvh.nodes.size();
        f.bvh_info.leaves = bvh.leaves;
        f.bvh_info.depth = bvh.depth;
        f.bvh_info.lane_stack = bvh.lane_stack;
        f.bvh_info.margin = (float)bvh.margin;
        f.bvh_info.origin_bound = bvh.obound;
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
        const uint32_t nl = std::min<uint32_t>(d->n_lights, RG_LB_MAX_LIGHTS);
        h.lbuf.assign(nl, RgLightBufDev{});
        int built = 0;
        for (uint32_t i = 0; i < nl; ++i) {
            RgLightBufBuild lb;
            if (!rg_build_lightbuf(sp.data(), (int)h.sph.size(), h.lights[i].kind, h.lights[i].dn, h.lights[i].v,
                                   bvh.extent, (double)bvh.obound, lb) ||
                !append_lightbuf(h, lb))
                continue;
            h.lbuf[i] = lb.dev;
            ++built;
        }
        // the camera buffer: a light buffer around the camera (ray.rs:53: every primary ray starts at
        // the origin), behind the lights' slots; primary rays test their direction's cell
        const double zero[3] = {0.0, 0.0, 0.0};
        RgLightBufBuild cam;
        if (rg_build_lightbuf(sp.data(), (int)h.sph.size(), RG_LIGHT_SPHERICAL, zero, zero, bvh.extent,
                              (double)bvh.obound, cam) &&
            append_lightbuf(h, cam)) {
            f.lb_cam = (int32_t)h.lbuf.size();
            h.lbuf.push_back(cam.dev);
        }
        if (!built && f.lb_cam < 0) h.lbuf.clear();
        f.n_lbuf = built ? (int32_t)nl : 0;
        f.n_lbdesc = (int32_t)h.lbuf.size();
        f.bvh_info.lbuf_bytes = (int64_t)((h.lb_ent.size() + h.lb_start.size()) * sizeof(uint32_t) +
                                          h.lbuf.size() * sizeof(RgLightBufDev));
    }
    // Shadow mask volume (rg_shadow_vol.cpp) over the sphere and plane tables in kernel order: scenes
    // the PLAIN light kernels can run (no disks, no boxes)
    if (RG_PLAIN_SHVOL != 0 && h.dsk.empty() && h.box.empty() && !nan_scene) {
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
            f.shvol_info.built = 1;
            f.shvol_info.g = sv.g;
            f.shvol_info.bytes = (int64_t)(sv.words.size() * sizeof(uint32_t));
            f.shvol_info.build_ms = sv.build_ms;
            f.shvol_info.set_share = sv.set_share;
            f.shvol_inv = sv.inv;
            f.shvol_off = sv.off;
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
    f.n_sph = (int32_t)h.sph.size();
    f.n_pln = (int32_t)h.pln.size();
    f.n_dsk = (int32_t)h.dsk.size();
    f.n_box = (int32_t)h.box.size();
    f.n_bodies = (int32_t)d->n_bodies;
    f.n_lights = (int32_t)d->n_lights;
    f.n_textures = (int32_t)d->n_textures;
    f.n_nodes = (int32_t)h.nodes.size();
    // the stack entry keeps the node index in its low RG_LANE_NODE_BITS bits; no tree, no walk
    f.lane_stack = (f.n_nodes > 0 && f.n_nodes <= (1 << RG_LANE_NODE_BITS) && bvh.lane_stack <= RG_LANE_STACK_MAX)
                       ? std::max(bvh.lane_stack, 1) : 0;
    return RG_OK;
}

rg_lds_layout rg_lds_layout_of(const rg_scene_facts &f, bool bvh, bool lbuf, uint32_t lstack_bytes) {
    auto al16 = [](uint32_t v) { return (v + 15u) & ~15u; };
    rg_lds_layout L;
    L.n_sph = (uint32_t)f.n_sph;
    L.n_nodes = bvh ? (uint32_t)f.n_nodes : 0u;
    L.lbuf_staged = lbuf ? 1u : 0u;
    L.sphf = lstack_bytes;
    L.sph = L.sphf + L.n_sph * (uint32_t)(sizeof(RgSphF) + sizeof(RgSphF2));
    L.cc = L.sph + L.n_sph * (uint32_t)sizeof(RgSph);
    L.nodes = al16(L.cc + L.n_sph * 8u);
    L.pln = L.nodes + L.n_nodes * (uint32_t)sizeof(RgBvhNode);
    L.dsk = L.pln + (uint32_t)f.n_pln * (uint32_t)sizeof(RgPln);
    L.box = L.dsk + (uint32_t)f.n_dsk * (uint32_t)sizeof(RgDsk);
    L.lights = al16(L.box + (uint32_t)f.n_box * (uint32_t)sizeof(RgBox));
    L.texs = L.lights + (uint32_t)f.n_lights * (uint32_t)sizeof(RgLightDev);
    L.lbuf = al16(L.texs + (uint32_t)f.n_textures * (uint32_t)sizeof(RgTexDev));
    L.bodies = L.lbuf + (lbuf ? (uint32_t)f.n_lbdesc * (uint32_t)sizeof(RgLightBufDev) : 0u);
    L.hot_bytes = L.bodies;
    L.mats = L.bodies + (uint32_t)f.n_bodies * (uint32_t)sizeof(RgBodyDev);
    L.total_bytes = L.mats + (uint32_t)f.n_bodies * (uint32_t)sizeof(RgMatDev);
    // behind the arena, in the blob image only: the PLAIN light kernels' tables (rg_device.h)
    L.texm = L.total_bytes;
    L.axes = L.texm + (uint32_t)f.n_textures * (uint32_t)sizeof(RgTexMagic);
    L.plain_bytes = L.axes + (uint32_t)f.n_bodies * (uint32_t)sizeof(RgPlnAxes);
    return L;
}

std::vector<unsigned char> rg_lds_image(const rg_host_tables &h, const std::vector<RgTexDev> &texs, const rg_lds_layout &L) {
    std::vector<unsigned char> img(L.plain_bytes, 0);
    auto put = [&](uint32_t off, const void *src, size_t bytes) {
        if (bytes && off + bytes <= img.size()) std::memcpy(img.data() + off, src, bytes);
    };
    put(L.sphf, h.sphf.data(), h.sphf.size() * sizeof(RgSphF));
    put(L.sphf + (uint32_t)(h.sphf.size() * sizeof(RgSphF)), h.sphf2.data(), h.sphf2.size() * sizeof(RgSphF2));
    put(L.sph, h.sph.data(), h.sph.size() * sizeof(RgSph));
    put(L.cc, h.sph_cc.data(), h.sph_cc.size() * sizeof(double));
    if (L.n_nodes > 0) put(L.nodes, h.nodes.data(), h.nodes.size() * sizeof(RgBvhNode));
    put(L.pln, h.pln.data(), h.pln.size() * sizeof(RgPln));
    put(L.dsk, h.dsk.data(), h.dsk.size() * sizeof(RgDsk));
    put(L.box, h.box.data(), h.box.size() * sizeof(RgBox));
    put(L.bodies, h.bodies.data(), h.bodies.size() * sizeof(RgBodyDev));
    put(L.mats, h.mats.data(), h.mats.size() * sizeof(RgMatDev));
    put(L.lights, h.lights.data(), h.lights.size() * sizeof(RgLightDev));
    put(L.texs, texs.data(), texs.size() * sizeof(RgTexDev));
    if (L.lbuf_staged) put(L.lbuf, h.lbuf.data(), h.lbuf.size() * sizeof(RgLightBufDev));
    // the PLAIN light kernels' tables: each texture dimension's magic, each plane's texture axes
    std::vector<RgTexMagic> texm(h.tex_w.size(), RgTexMagic{0, 0, 0, 0});
    for (size_t t = 0; t < texm.size(); ++t) {
        if (h.tex_w[t] == 0 || h.tex_h[t] == 0) continue;
        const RgMagicU32 mw = rg_magic_u32(h.tex_w[t]), mh = rg_magic_u32(h.tex_h[t]);
        texm[t] = RgTexMagic{mw.m, mw.sh, mh.m, mh.sh};
    }
    put(L.texm, texm.data(), texm.size() * sizeof(RgTexMagic));
    std::vector<RgPlnAxes> axes(h.bodies.size());
    std::memset(axes.data(), 0, axes.size() * sizeof(RgPlnAxes));
    for (size_t b = 0; b < axes.size(); ++b)
        if (h.bodies[b].kind == RG_BODY_PLANE) rg_plane_axes(&h.bodies[b].p[3], axes[b].xa, axes[b].ya);
    put(L.axes, axes.data(), axes.size() * sizeof(RgPlnAxes));
    return img;
}
