/* camera_oracle.c — the reference for camera frames (tests/camera_ref.py builds and loads it; nothing
 * in raingun_amd/ may).  The pinned oracle as it stands, plus ONE function: rgo_render's pixel loop
 * with the camera ray of include/raingun.h (rg_camera) in place of create_prime.  It reuses the
 * oracle's static ray_new, trace and get_color; same tilings, rgb output, counts and first error
 * pixel.  tests/test_camera_cpu.py ties it back to rgo_render: with the identity camera it gives
 * rgo_render's bytes, counts and status, and with the camera turned 180 degrees about y it gives, on
 * the scene mirrored in x and z, rgo_render's frame of the original scene. */
#include "../../oracle/raingun_oracle.c"

/* One thread (the frames of the tests are small); nthreads of rgo_render has no counterpart. */
int32_t rgc_render(const rg_scene_desc *s, uint32_t w, uint32_t h, const rg_tiling *tiling, const rg_camera *cam,
                   uint8_t *rgba, float *rgb, rg_ray_counts *counts, int64_t *error_pixel) {
    if (!s || !rgba || !cam || w == 0 || h == 0) return RG_ERR_INVALID_ARGUMENT;
    if (w < h) return RG_ERR_PORTRAIT; /* ray.rs:42 */
    rg_tiling whole = {h, 1, 0};
    if (!tiling) tiling = &whole;
    if (tiling->tile_rows == 0 || tiling->tile_stride == 0 || tiling->tile_offset >= tiling->tile_stride)
        return RG_ERR_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < s->n_bodies; ++i) {
        const rg_material *m = &s->bodies[i].material;
        if (m->coloration == RG_COLORATION_TEXTURE &&
            (m->texture < 0 || (uint32_t)m->texture >= s->n_textures || !s->textures[m->texture].rgba ||
             s->textures[m->texture].width == 0 || s->textures[m->texture].height == 0))
            return RG_ERR_TEXTURE;
    }
    ctx_t c = {s, rgo_fov_adjustment(s->fov)};
    const v3 eye = p3(cam->eye), right = p3(cam->right), up = p3(cam->up), fwd = p3(cam->forward);
    rg_ray_counts total = {0, 0, 0};
    int64_t err_pixel = -1;
    int32_t err_code = 0;
    const uint32_t n_out_rows = rgo_tiling_rows(h, tiling);
    for (uint32_t orow = 0; orow < n_out_rows; ++orow) {
        uint32_t tile_local = orow / tiling->tile_rows, r_in_tile = orow % tiling->tile_rows;
        uint64_t tile = (uint64_t)tile_local * tiling->tile_stride + tiling->tile_offset;
        uint64_t y64 = tile * tiling->tile_rows + r_in_tile;
        uint8_t *orgba = rgba + (size_t)orow * w * 4;
        float *orgb = rgb ? rgb + (size_t)orow * w * 3 : NULL;
        if (y64 >= h) { /* padding rows of a partial last tile */
            memset(orgba, 0, (size_t)w * 4);
            if (orgb) memset(orgb, 0, (size_t)w * 12);
            continue;
        }
        uint32_t y = (uint32_t)y64;
        for (uint32_t x = 0; x < w; ++x) {
            pix_t px;
            memset(&px, 0, sizeof px);
            /* the sensor coordinates of create_prime (ray.rs:43-51), then the camera's basis */
            double aspect = (double)w / (double)h;
            double sx = ((((double)x + 0.5) / (double)w) * 2.0 - 1.0) * aspect * c.fov_adjustment;
            double sy = (1.0 - (((double)y + 0.5) / (double)h) * 2.0) * c.fov_adjustment;
            v3 D = v3_make((right.x * sx + up.x * sy) + fwd.x, (right.y * sx + up.y * sy) + fwd.y,
                           (right.z * sx + up.z * sy) + fwd.z);
            ray_t r = ray_new(eye, v3_normalize(D));
            double d;
            int32_t bi;
            col cc;
            px.counts.primary++;
            if (trace(&c, &r, &d, &bi, &px)) cc = get_color(&c, &r, d, bi, 0, &px);
            else cc = col_make(s->default_color[0], s->default_color[1], s->default_color[2]);
            total.primary += px.counts.primary;
            total.shadow += px.counts.shadow;
            total.secondary += px.counts.secondary;
            int64_t lin = (int64_t)y * w + x;
            if (px.err && (err_pixel < 0 || lin < err_pixel)) { err_pixel = lin; err_code = px.err; }
            orgba[4 * x + 0] = rgo_f32_to_u8(cc.r * 255.0f); /* color.rs:32-37 */
            orgba[4 * x + 1] = rgo_f32_to_u8(cc.g * 255.0f);
            orgba[4 * x + 2] = rgo_f32_to_u8(cc.b * 255.0f);
            orgba[4 * x + 3] = 255;
            if (orgb) { orgb[3 * x] = cc.r; orgb[3 * x + 1] = cc.g; orgb[3 * x + 2] = cc.b; }
        }
    }
    if (counts) *counts = total;
    if (error_pixel) *error_pixel = err_pixel;
    return err_pixel >= 0 ? err_code : RG_OK;
}
