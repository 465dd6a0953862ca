/* lens_oracle.c — the reference for frames through a thin lens (tests/lens_ref.py builds and loads it;
 * nothing in raingun_amd/ may).  The pinned oracle as it stands, plus ONE function: the pixel loop of
 * camera_oracle.c over the kW x kH sample frame, with the lens ray of include/raingun.h (rg_lens) in place
 * of the camera ray.  The two tables (rg_lens_tables) are the caller's: no transcendental is evaluated
 * here.  It reuses the oracle's static ray_new, trace and get_color; rgb output, counts and first error
 * pixel (of the sample frame) as rgo_render.  tests/test_lens_cpu.py ties it back to the camera reference:
 * with an all-zero points table and focus 1 it gives rgc_render's bytes at (kW, kH). */
#include "../../oracle/raingun_oracle.c"

static v3 lens_axis(v3 a, double aperture) { /* normalize(a) * aperture */
    v3 n = v3_normalize(a);
    return v3_make(n.x * aperture, n.y * aperture, n.z * aperture);
}

static uint32_t lowbias32(uint32_t n) {
    n ^= n >> 16;
    n *= 0x7feb352du;
    n ^= n >> 15;
    n *= 0x846ca68bu;
    n ^= n >> 16;
    return n;
}

/* w, h: the OUTPUT frame; k x k samples per pixel; rgba / rgb: the (k h) x (k w) sample frame.
 * points: 2 k^2 doubles, rotations: 128 doubles. */
int32_t rgl_render(const rg_scene_desc *s, uint32_t w, uint32_t h, uint32_t k, const rg_camera *cam, double aperture,
                   double focus, const double *points, const double *rotations, uint8_t *rgba, float *rgb,
                   rg_ray_counts *counts, int64_t *error_pixel) {
    if (!s || !rgba || !cam || !points || !rotations || w == 0 || h == 0 || k == 0) return RG_ERR_INVALID_ARGUMENT;
    if (w < h) return RG_ERR_PORTRAIT; /* ray.rs:42 */
    for (uint32_t i = 0; i < s->n_bodies; ++i) {
        const rg_material *m = &s->bodies[i].material;
        if (m->coloration == RG_COLORATION_TEXTURE &&
            (m->texture < 0 || (uint32_t)m->texture >= s->n_textures || !s->textures[m->texture].rgba ||
             s->textures[m->texture].width == 0 || s->textures[m->texture].height == 0))
            return RG_ERR_TEXTURE;
    }
    ctx_t c = {s, rgo_fov_adjustment(s->fov)};
    const v3 eye = p3(cam->eye), right = p3(cam->right), up = p3(cam->up), fwd = p3(cam->forward);
    const v3 LR = lens_axis(right, aperture), LU = lens_axis(up, aperture);
    const uint32_t kw = k * w, kh = k * h;
    rg_ray_counts total = {0, 0, 0};
    int64_t err_pixel = -1;
    int32_t err_code = 0;
    for (uint32_t y = 0; y < kh; ++y) {
        uint8_t *orgba = rgba + (size_t)y * kw * 4;
        float *orgb = rgb ? rgb + (size_t)y * kw * 3 : NULL;
        for (uint32_t x = 0; x < kw; ++x) {
            pix_t px;
            memset(&px, 0, sizeof px);
            /* the sensor coordinates of create_prime (ray.rs:43-51) on the sample frame, the camera's basis */
            double aspect = (double)kw / (double)kh;
            double sx = ((((double)x + 0.5) / (double)kw) * 2.0 - 1.0) * aspect * c.fov_adjustment;
            double sy = (1.0 - (((double)y + 0.5) / (double)kh) * 2.0) * c.fov_adjustment;
            v3 D = v3_make((right.x * sx + up.x * sy) + fwd.x, (right.y * sx + up.y * sy) + fwd.y,
                           (right.z * sx + up.z * sy) + fwd.z);
            /* the sample's point of the lens disk, turned by the output pixel's hash */
            uint32_t sidx = (y % k) * k + (x % k);
            uint32_t hsh = lowbias32((y / k) * w + (x / k));
            double pu = points[2 * sidx], pv = points[2 * sidx + 1];
            double cr = rotations[2 * (hsh & 63u)], sr = rotations[2 * (hsh & 63u) + 1];
            double qu = cr * pu - sr * pv, qv = sr * pu + cr * pv;
            v3 O = v3_make(LR.x * qu + LU.x * qv, LR.y * qu + LU.y * qv, LR.z * qu + LU.z * qv);
            v3 origin = v3_make(eye.x + O.x, eye.y + O.y, eye.z + O.z);
            v3 V = v3_make(D.x * focus - O.x, D.y * focus - O.y, D.z * focus - O.z);
            ray_t r = ray_new(origin, v3_normalize(V));
            double d;
            int32_t bi;
            col cc;
            px.counts.primary++;
            if (trace(&c, &r, &d, &bi, &px)) cc = get_color(&c, &r, d, bi, 0, &px);
            else cc = col_make(s->default_color[0], s->default_color[1], s->default_color[2]);
            total.primary += px.counts.primary;
            total.shadow += px.counts.shadow;
            total.secondary += px.counts.secondary;
            int64_t lin = (int64_t)y * kw + x;
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
