// scene_build_shim.cpp — the host scene builder (raingun_amd/csrc/rg_scene_build.cpp) behind a C
// interface for tests/test_scene_build_cpu.py: build a description, then read every host table,
// the facts, an arena layout and an arena image as bytes.  Built as a shared library with plain
// g++ together with rg_scene_build.cpp and the three builders it calls; no device is involved.
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../raingun_amd/csrc/rg_scene_tables.h"

namespace {

struct Build {
    rg_host_tables h;
    rg_scene_facts f;
    std::vector<RgTexDev> texs;  // descriptors as an upload would make them, with made-up texel addresses
};

template <class T>
const void *bytes_of(const std::vector<T> &v, uint64_t *n) {
    *n = v.size() * sizeof(T);
    return v.data();
}

}  // namespace

extern "C" {

// A build of `d` (free with sb_free), or null with the builder's status in *status.
void *sb_build(const rg_scene_desc *d, int32_t *status) {
    Build *b = new Build();
    *status = (int32_t)rg_scene_build(d, b->h, b->f);
    if (*status != RG_OK) {
        delete b;
        return nullptr;
    }
    b->texs.resize(b->h.tex_w.size());
    for (size_t i = 0; i < b->texs.size(); ++i) {
        b->texs[i].texels = b->h.texels[i].empty() ? nullptr : reinterpret_cast<const uint32_t *>((uintptr_t)(0x10000 * (i + 1)));
        b->texs[i].w = (int32_t)b->h.tex_w[i];
        b->texs[i].h = (int32_t)b->h.tex_h[i];
    }
    return b;
}

void sb_free(void *p) { delete static_cast<Build *>(p); }

// The bytes of table `name` ("facts" and "texs" included); null for an unknown name.
const void *sb_table(const void *p, const char *name, uint64_t *n) {
    const Build *b = static_cast<const Build *>(p);
    const rg_host_tables &h = b->h;
    const std::string k = name;
    *n = 0;
#define SB_T(x) if (k == #x) return bytes_of(h.x, n)
    SB_T(sph); SB_T(sphf); SB_T(sphf2); SB_T(sph_cc); SB_T(sph_id); SB_T(pln_id); SB_T(dsk_id); SB_T(box_id);
    SB_T(pln); SB_T(dsk); SB_T(box); SB_T(bodies); SB_T(mats); SB_T(lights); SB_T(nodes); SB_T(lbuf);
    SB_T(lb_start); SB_T(lb_ent); SB_T(shvol); SB_T(tex_w); SB_T(tex_h);
#undef SB_T
    if (k == "texs") return bytes_of(b->texs, n);
    if (k == "facts") {
        *n = sizeof b->f;
        return &b->f;
    }
    if (k.rfind("texels", 0) == 0) {  // "texels<i>"
        const size_t i = (size_t)std::stoul(k.substr(6));
        if (i < h.texels.size()) return bytes_of(h.texels[i], n);
    }
    return nullptr;
}

uint32_t sb_layout_words(void) { return (uint32_t)(sizeof(rg_lds_layout) / sizeof(uint32_t)); }

void sb_layout(const void *p, int32_t bvh, int32_t lbuf, uint32_t lstack_bytes, uint32_t *out) {
    const rg_lds_layout L = rg_lds_layout_of(static_cast<const Build *>(p)->f, bvh != 0, lbuf != 0, lstack_bytes);
    std::memcpy(out, &L, sizeof L);
}

// The arena image of that layout into out[0 .. cap); returns its size (nothing written if cap is smaller).
uint64_t sb_image(const void *p, int32_t bvh, int32_t lbuf, uint32_t lstack_bytes, uint8_t *out, uint64_t cap) {
    const Build *b = static_cast<const Build *>(p);
    const rg_lds_layout L = rg_lds_layout_of(b->f, bvh != 0, lbuf != 0, lstack_bytes);
    const std::vector<unsigned char> img = rg_lds_image(b->h, b->texs, L);
    if (img.size() <= cap && !img.empty()) std::memcpy(out, img.data(), img.size());
    return img.size();
}

}  // extern "C"
