// rg_ambient.hip — the ambient term's entry points of the C ABI: rg_ao_filter /
// rg_ao_filter_async (the edge-stopping filter of the AO pass alone) and rg_render_image_ambient /
// rg_render_ambient_async (the beauty frame, the AOV pass, the AO pass, the filter and the compose, in that order
// on one stream).  Host code only: the two image kernels and their launchers are rg_ao_filter.hip's, the tracing
// passes are called through their own entry points, so no kernel is built differently for this file.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/raingun.h"
#include "rg_ambient.h"
#include "rg_ao.h"
#include "rg_internal.h"
#include "rg_launchers.h"

namespace {

bool filter_args_ok(const void *ao, const void *body, const void *normal, uint32_t W, uint32_t H,
                    const rg_ao_filter_desc *f, const void *out) {
    if ((reinterpret_cast<uintptr_t>(ao) | reinterpret_cast<uintptr_t>(body) | reinterpret_cast<uintptr_t>(normal) |
         reinterpret_cast<uintptr_t>(out)) & 3u)
        return false;
    return ao && body && normal && out && out != ao && W != 0 && H != 0 && f &&
           (unsigned long long)W * H < (1ull << 32) && rg_ao_filter_valid(f->radius, f->normal_min);
}

rg_status ambient_check(const rg_scene *s, uint32_t W, uint32_t H, const rg_ambient *m, const void *rgba) {
    if (!s || !m || !rgba || W == 0 || H == 0) return RG_ERR_INVALID_ARGUMENT;
    if (!rg_ambient_valid(m->color, m->samples, m->filter_radius, m->normal_min) ||
        !rg_ao_valid(m->ao.samples, m->ao.radius, m->ao.bias))
        return RG_ERR_INVALID_ARGUMENT;
    if ((unsigned long long)m->samples * W * ((unsigned long long)m->samples * H) >= (1ull << 32))
        return RG_ERR_INVALID_ARGUMENT;
    if (W < H) return RG_ERR_PORTRAIT;
    return RG_OK;
}

bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// The scene's share table on its device, made on the first ambient frame (no body: one float, nothing copied).
rg_status share_table(const rg_scene *s) {
    const std::vector<float> &h = s->host->amb_share;
    return rg_table_once(s, s->d_share, h.empty() ? nullptr : h.data(), (h.empty() ? 1 : h.size()) * sizeof(float));
}

// The stream's resource set with at least `bytes` of scratch (nullptr: out of memory / device error).  A set is
// kept only once it is whole: a stream whose first frame fails leaves nothing behind.  A kept set lives until
// rg_scene_release_stream of its stream, the null stream's until the scene is destroyed.
rg_ambient_res *ambient_res(const rg_scene *s, hipStream_t hs, size_t bytes, rg_status *st) {
    for (rg_ambient_res &c : s->amb)
        if (c.stream == hs) return (*st = rg_grow(RG_MEM_DEVICE, c.mem, c.cap, bytes)) == RG_OK ? &c : nullptr;
    rg_ambient_res c;
    c.stream = hs;
    *st = ok(hipEventCreate(&c.ev0)) && ok(hipEventCreate(&c.ev1)) ? RG_OK : RG_ERR_DEVICE;
    if (*st == RG_OK) *st = rg_grow(RG_MEM_DEVICE, c.mem, c.cap, bytes);
    if (*st != RG_OK) {
        if (c.ev0) (void)hipEventDestroy(c.ev0);
        if (c.ev1) (void)hipEventDestroy(c.ev1);
        return nullptr;
    }
    s->amb.push_back(c);
    return &s->amb.back();
}

size_t align256(size_t n) { return (n + 255u) & ~(size_t)255u; }

}  // namespace

void rg_ambient_release(const rg_scene *s, hipStream_t stream, bool all) {
    for (size_t i = 0; i < s->amb.size();) {
        rg_ambient_res &c = s->amb[i];
        if (!all && c.stream != stream) {
            ++i;
            continue;
        }
        if (c.mem) (void)hipFree(c.mem);  // waits for the device
        if (c.ev0) (void)hipEventDestroy(c.ev0);
        if (c.ev1) (void)hipEventDestroy(c.ev1);
        s->amb.erase(s->amb.begin() + (std::ptrdiff_t)i);
    }
}

extern "C" {

rg_status rg_ao_filter_async(int32_t device, const float *ao_dev, const int32_t *body_dev, const float *normal_dev,
                             uint32_t width, uint32_t height, const rg_ao_filter_desc *filter, float *ao_out_dev,
                             void *stream) {
    if (device < 0 || !filter_args_ok(ao_dev, body_dev, normal_dev, width, height, filter, ao_out_dev))
        return RG_ERR_INVALID_ARGUMENT;
    if (!ok(hipSetDevice(device))) return RG_ERR_DEVICE;
    if (!ok(rg_launch_ao_filter(ao_dev, body_dev, normal_dev, width, height, filter->radius, filter->normal_min,
                                ao_out_dev, static_cast<hipStream_t>(stream))))
        return RG_ERR_DEVICE;
    return RG_OK;
}

rg_status rg_ao_filter(int32_t device, const float *ao_in, const int32_t *body, const float *normal, uint32_t width,
                       uint32_t height, const rg_ao_filter_desc *filter, float *ao_out) {
    if (device < 0 || !filter_args_ok(ao_in, body, normal, width, height, filter, ao_out)) return RG_ERR_INVALID_ARGUMENT;
    if (!ok(hipSetDevice(device))) return RG_ERR_DEVICE;
    const size_t px = (size_t)width * height;
    rg_scratch mem;
    float *d_ao = mem.dev<float>(px * 4);
    int32_t *d_body = mem.dev<int32_t>(px * 4);
    float *d_n = mem.dev<float>(px * 12), *d_out = mem.dev<float>(px * 4);
    if (mem.status() != RG_OK) return mem.status();
    if (!ok(hipMemcpy(d_ao, ao_in, px * 4, hipMemcpyHostToDevice)) ||
        !ok(hipMemcpy(d_body, body, px * 4, hipMemcpyHostToDevice)) ||
        !ok(hipMemcpy(d_n, normal, px * 12, hipMemcpyHostToDevice)) ||
        !ok(rg_launch_ao_filter(d_ao, d_body, d_n, width, height, filter->radius, filter->normal_min, d_out, nullptr)) ||
        !ok(hipMemcpy(ao_out, d_out, px * 4, hipMemcpyDeviceToHost)))
        return RG_ERR_DEVICE;
    return RG_OK;
}

rg_status rg_render_ambient_async(const rg_scene *s, uint32_t width, uint32_t height, const rg_ambient *m,
                                  uint8_t *rgba_dev, float *rgb_dev, float *ao_dev, void *stream, rg_stats *stats) {
    rg_status st = ambient_check(s, width, height, m, rgba_dev);
    if (st != RG_OK) return st;
    if (!aligned4(rgba_dev) || !aligned4(rgb_dev) || !aligned4(ao_dev)) return RG_ERR_INVALID_ARGUMENT;
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    if ((st = share_table(s)) != RG_OK) return st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const size_t px = (size_t)width * height;
    // scratch: albedo, normal, body, the raw pass, and what the caller does not take: rgb and the filtered pass
    const size_t b3 = align256(px * 12), b1 = align256(px * 4);
    const bool filtered = m->filter_radius > 0;
    rg_ambient_res *r = ambient_res(s, hs, 2 * b3 + 2 * b1 + (rgb_dev ? 0 : b3) + (ao_dev ? 0 : b1), &st);
    if (!r) return st;
    char *at = static_cast<char *>(r->mem);
    float *albedo = reinterpret_cast<float *>(at);
    float *normal = reinterpret_cast<float *>(at + b3);
    int32_t *body = reinterpret_cast<int32_t *>(at + 2 * b3);
    float *raw = reinterpret_cast<float *>(at + 2 * b3 + b1);
    at += 2 * b3 + 2 * b1;
    float *rgb = rgb_dev ? rgb_dev : reinterpret_cast<float *>(at);
    if (!rgb_dev) at += b3;
    float *aof = ao_dev ? ao_dev : reinterpret_cast<float *>(at);
    if (!filtered) raw = aof;  // the raw pass is the one composed (and delivered)

    rg_stats pass[3];
    const rg_tiling whole = {height, 1, 0};
    const rg_aov layers = {body, nullptr, normal, nullptr, albedo};
    rg_status pst[3];
    pst[0] = rg_render_aa_async(s, width, height, m->samples, rgba_dev, rgb, stream, stats ? &pass[0] : nullptr);
    if (!rg_delivers_frame(pst[0])) return pst[0];
    pst[1] = rg_render_aov_async(s, width, height, &whole, &layers, stream, stats ? &pass[1] : nullptr);
    if (!rg_delivers_frame(pst[1])) return pst[1];
    pst[2] = rg_render_ao_async(s, width, height, &whole, &m->ao, raw, stream, stats ? &pass[2] : nullptr);
    if (!rg_delivers_frame(pst[2])) return pst[2];

    if (stats && !ok(hipEventRecord(r->ev0, hs))) return RG_ERR_DEVICE;
    if (filtered && !ok(rg_launch_ao_filter(raw, body, normal, width, height, m->filter_radius, m->normal_min, aof, hs)))
        return RG_ERR_DEVICE;
    if (!ok(rg_launch_ambient_compose(rgb, albedo, body, aof, s->d_share, (uint32_t)s->host->amb_share.size(), m->color,
                                      px, rgba_dev, rgb_dev, hs)))
        return RG_ERR_DEVICE;
    if (!stats) return RG_OK;
    if (!ok(hipEventRecord(r->ev1, hs)) || !ok(hipStreamSynchronize(hs))) return RG_ERR_DEVICE;
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, r->ev0, r->ev1);
    rg_stats total{};
    total.kernel_ms = pass[0].kernel_ms + pass[1].kernel_ms + pass[2].kernel_ms + ms;
    total.error_pixel = -1;
    st = RG_OK;
    for (int i = 0; i < 3; ++i) rg_stats_add(total, st, pass[i], pst[i]);  // a tie keeps the earlier pass's
    *stats = total;
    return st;
}

rg_status rg_render_image_ambient(const rg_scene *s, uint32_t width, uint32_t height, const rg_ambient *m,
                                  uint8_t *rgba_out, float *rgb_out, float *ao_out, rg_stats *stats) {
    rg_status st = ambient_check(s, width, height, m, rgba_out);
    if (st != RG_OK) return st;
    if (!ok(hipSetDevice(s->device))) return RG_ERR_DEVICE;
    const size_t px = (size_t)width * height;
    rg_scratch mem;
    uint8_t *d_rgba = mem.dev<uint8_t>(px * 4);
    float *d_rgb = rgb_out ? mem.dev<float>(px * 12) : nullptr;
    float *d_ao = ao_out ? mem.dev<float>(px * 4) : nullptr;
    if (mem.status() != RG_OK) return mem.status();
    rg_stats local;
    st = rg_render_ambient_async(s, width, height, m, d_rgba, d_rgb, d_ao, nullptr, stats ? stats : &local);
    // the frame is delivered on the reference's panics too
    if (rg_delivers_frame(st) &&
        (!ok(hipMemcpy(rgba_out, d_rgba, px * 4, hipMemcpyDeviceToHost)) ||
         (rgb_out && !ok(hipMemcpy(rgb_out, d_rgb, px * 12, hipMemcpyDeviceToHost))) ||
         (ao_out && !ok(hipMemcpy(ao_out, d_ao, px * 4, hipMemcpyDeviceToHost)))))
        st = RG_ERR_DEVICE;
    return st;
}

}  // extern "C"
