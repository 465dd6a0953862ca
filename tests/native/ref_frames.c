/* ref_frames.c — the reference for camera frames, AOV layers and frames through a thin lens
 * (tests/ref_lib.py builds and loads it; nothing in raingun_amd/ may).  The pinned oracle as it stands, plus
 * ONE pixel loop (rgo_render's: frame check, row walk, first error pixel) under three entries:
 *   rgc_render  the camera ray of include/raingun.h (rg_camera) in place of create_prime;
 *   rgl_render  the lens ray (rg_lens) over the kW x kH sample frame; the two tables (rg_lens_tables) are
 *               the caller's: no transcendental is evaluated here;
 *   rga_render  create_prime or the camera ray, stopping after the primary hit and writing what it found.
 * It reuses the oracle's static ray_new, create_prime, trace, get_color, surface_normal, texture_coords and
 * material_color.  tests/test_camera_cpu.py ties the loop back to rgo_render (identity camera; the camera
 * turned 180 degrees about y on the scene mirrored in x and z), tests/test_aov_cpu.py to rgo_trace and
 * rgo_render, tests/test_lens_cpu.py the lens entry to the camera entry at (kW, kH).
 * One thread (the frames of the tests are small); nthreads of rgo_render has no counterpart. */
#include "../../oracle/raingun_oracle.c"

typedef struct {
    ctx_t c;
    uint32_t w, h;        /* the frame being walked: the sample frame for the lens */
    const rg_camera *cam; /* NULL: create_prime (AOV only) */
    v3 eye, right, up, fwd;
    rg_ray_counts total;
    int64_t err_pixel;
    int32_t err_code;
    uint8_t *rgba; /* colour entries */
    float *rgb;
    uint32_t k; /* lens */
    double focus;
    v3 LR, LU;
    const double *points, *rotations;
    int32_t *body; /* AOV layers, each nullable */
    double *depth;
    float *normal, *uv, *albedo;
} frame_t;

/* The checks of rgo_render in its order (the first failing one decides the status); `entry_ok` carries the
 * entry's own argument conditions. */
static int32_t frame_check(const rg_scene_desc *s, int entry_ok, uint32_t w, uint32_t h, const rg_tiling *tiling) {
    if (!s || !entry_ok || w == 0 || h == 0) return RG_ERR_INVALID_ARGUMENT;
    if (w < h) return RG_ERR_PORTRAIT; /* ray.rs:42 */
    if (tiling->tile_rows == 0 || tiling->tile_stride == 0 || tiling->tile_offset >= tiling->tile_stride)
        return RG_ERR_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < s->n_bodies; ++i) {
        const rg_material *m = &s->bodies[i].material;
        if (m->coloration == RG_COLORATION_TEXTURE &&
            (m->texture < 0 || (uint32_t)m->texture >= s->n_textures || !s->textures[m->texture].rgba ||
             s->textures[m->texture].width == 0 || s->textures[m->texture].height == 0))
            return RG_ERR_TEXTURE;
    }
    return RG_OK;
}

static void frame_init(frame_t *f, const rg_scene_desc *s, uint32_t w, uint32_t h, const rg_camera *cam) {
    memset(f, 0, sizeof *f);
    f->c.s = s; f->c.fov_adjustment = rgo_fov_adjustment(s->fov);
    f->w = w; f->h = h; f->cam = cam;
    if (cam) { f->eye = p3(cam->eye); f->right = p3(cam->right); f->up = p3(cam->up); f->fwd = p3(cam->forward); }
    f->err_pixel = -1;
}

/* The sensor coordinates of create_prime (ray.rs:43-51), then the camera's basis: the ray's direction
 * before it is normalised. */
static v3 camera_dir(const frame_t *f, uint32_t x, uint32_t y) {
    double aspect = (double)f->w / (double)f->h;
    double sx = ((((double)x + 0.5) / (double)f->w) * 2.0 - 1.0) * aspect * f->c.fov_adjustment;
    double sy = (1.0 - (((double)y + 0.5) / (double)f->h) * 2.0) * f->c.fov_adjustment;
    return v3_make((f->right.x * sx + f->up.x * sy) + f->fwd.x, (f->right.y * sx + f->up.y * sy) + f->fwd.y,
                   (f->right.z * sx + f->up.z * sy) + f->fwd.z);
}

static ray_t camera_ray(const frame_t *f, uint32_t x, uint32_t y) {
    return ray_new(f->eye, v3_normalize(camera_dir(f, x, y)));
}

/* The error pixel is the lowest linear index of the frame being walked. */
static void note_error(frame_t *f, uint32_t x, uint32_t y, const pix_t *px) {
    int64_t lin = (int64_t)y * f->w + x;
    if (px->err && (f->err_pixel < 0 || lin < f->err_pixel)) { f->err_pixel = lin; f->err_code = px->err; }
}

/* Output row -> (tile, row in tile) -> image row, or a padding row of a partial last tile; `o` is the
 * pixel's linear index in the output. */
static int32_t walk_frame(frame_t *f, const rg_tiling *tiling, void (*pixel)(frame_t *, size_t o, uint32_t x, uint32_t y),
                          void (*padding)(frame_t *, size_t o), rg_ray_counts *counts, int64_t *error_pixel) {
    const uint32_t n_out_rows = rgo_tiling_rows(f->h, tiling);
    for (uint32_t orow = 0; orow < n_out_rows; ++orow) {
        uint32_t tile_local = orow / tiling->tile_rows, r_in_tile = orow % tiling->tile_rows;
        uint64_t tile = (uint64_t)tile_local * tiling->tile_stride + tiling->tile_offset;
        uint64_t y64 = tile * tiling->tile_rows + r_in_tile;
        for (uint32_t x = 0; x < f->w; ++x) {
            size_t o = (size_t)orow * f->w + x;
            if (y64 >= f->h) padding(f, o);
            else pixel(f, o, x, (uint32_t)y64);
        }
    }
    if (counts) *counts = f->total;
    if (error_pixel) *error_pixel = f->err_pixel;
    return f->err_pixel >= 0 ? f->err_code : RG_OK;
}

/* ------------------------------------------------------------ the colour entries */
static void colour_padding(frame_t *f, size_t o) {
    memset(f->rgba + 4 * o, 0, 4);
    if (f->rgb) memset(f->rgb + 3 * o, 0, 12);
}

/* rgo_render's pixel from the primary ray on (rendering.rs:71-78, then the worker's tail). */
static void colour_pixel(frame_t *f, size_t o, uint32_t x, uint32_t y, ray_t r) {
    const rg_scene_desc *s = f->c.s;
    pix_t px;
    memset(&px, 0, sizeof px);
    double d;
    int32_t bi;
    col cc;
    px.counts.primary++;
    if (trace(&f->c, &r, &d, &bi, &px)) cc = get_color(&f->c, &r, d, bi, 0, &px);
    else cc = col_make(s->default_color[0], s->default_color[1], s->default_color[2]);
    f->total.primary += px.counts.primary;
    f->total.shadow += px.counts.shadow;
    f->total.secondary += px.counts.secondary;
    note_error(f, x, y, &px);
    f->rgba[4 * o + 0] = rgo_f32_to_u8(cc.r * 255.0f); /* color.rs:32-37 */
    f->rgba[4 * o + 1] = rgo_f32_to_u8(cc.g * 255.0f);
    f->rgba[4 * o + 2] = rgo_f32_to_u8(cc.b * 255.0f);
    f->rgba[4 * o + 3] = 255;
    if (f->rgb) { f->rgb[3 * o] = cc.r; f->rgb[3 * o + 1] = cc.g; f->rgb[3 * o + 2] = cc.b; }
}

static void camera_pixel(frame_t *f, size_t o, uint32_t x, uint32_t y) { colour_pixel(f, o, x, y, camera_ray(f, x, y)); }

int32_t rgc_render(const rg_scene_desc *s, uint32_t w, uint32_t h, const rg_tiling *tiling, const rg_camera *cam,
                   uint8_t *rgba, float *rgb, rg_ray_counts *counts, int64_t *error_pixel) {
    rg_tiling whole = {h, 1, 0};
    if (!tiling) tiling = &whole;
    int32_t st = frame_check(s, rgba && cam, w, h, tiling);
    if (st != RG_OK) return st;
    frame_t f;
    frame_init(&f, s, w, h, cam);
    f.rgba = rgba; f.rgb = rgb;
    return walk_frame(&f, tiling, camera_pixel, colour_padding, counts, error_pixel);
}

/* ------------------------------------------------------------ the lens */
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

static void lens_pixel(frame_t *f, size_t o, uint32_t x, uint32_t y) {
    const uint32_t k = f->k;
    v3 D = camera_dir(f, x, y);
    /* the sample's point of the lens disk, turned by the output pixel's hash */
    uint32_t sidx = (y % k) * k + (x % k);
    uint32_t hsh = lowbias32((y / k) * (f->w / k) + (x / k));
    double pu = f->points[2 * sidx], pv = f->points[2 * sidx + 1];
    double cr = f->rotations[2 * (hsh & 63u)], sr = f->rotations[2 * (hsh & 63u) + 1];
    double qu = cr * pu - sr * pv, qv = sr * pu + cr * pv;
    v3 O = v3_make(f->LR.x * qu + f->LU.x * qv, f->LR.y * qu + f->LU.y * qv, f->LR.z * qu + f->LU.z * qv);
    v3 origin = v3_make(f->eye.x + O.x, f->eye.y + O.y, f->eye.z + O.z);
    v3 V = v3_make(D.x * f->focus - O.x, D.y * f->focus - O.y, D.z * f->focus - O.z);
    colour_pixel(f, o, x, y, ray_new(origin, v3_normalize(V)));
}

/* w, h: the OUTPUT frame; k x k samples per pixel; rgba / rgb: the (k h) x (k w) sample frame, walked whole.
 * points: 2 k^2 doubles, rotations: 128 doubles. */
int32_t rgl_render(const rg_scene_desc *s, uint32_t w, uint32_t h, uint32_t k, const rg_camera *cam, double aperture,
                   double focus, const double *points, const double *rotations, uint8_t *rgba, float *rgb,
                   rg_ray_counts *counts, int64_t *error_pixel) {
    const rg_tiling whole = {k * h, 1, 0};
    int32_t st = frame_check(s, rgba && cam && points && rotations && k != 0, w, h, &whole);
    if (st != RG_OK) return st;
    frame_t f;
    frame_init(&f, s, k * w, k * h, cam);
    f.rgba = rgba; f.rgb = rgb;
    f.k = k; f.focus = focus; f.points = points; f.rotations = rotations;
    f.LR = lens_axis(f.right, aperture); f.LU = lens_axis(f.up, aperture);
    return walk_frame(&f, &whole, lens_pixel, colour_padding, counts, error_pixel);
}

/* ------------------------------------------------------------ AOV layers */
static void aov_store(frame_t *f, size_t o, int32_t bi, double d, const float *n3, const float *t2, const float *a3) {
    if (f->body) f->body[o] = bi;
    if (f->depth) f->depth[o] = d;
    if (f->normal) memcpy(f->normal + 3 * o, n3, 3 * sizeof *n3);
    if (f->uv) memcpy(f->uv + 2 * o, t2, 2 * sizeof *t2);
    if (f->albedo) memcpy(f->albedo + 3 * o, a3, 3 * sizeof *a3);
}

/* Padding rows of a partial last tile: body -1, depth +inf, zeros elsewhere. */
static void aov_padding(frame_t *f, size_t o) {
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    aov_store(f, o, -1, INFINITY, zero, zero, zero);
}

static void aov_pixel(frame_t *f, size_t o, uint32_t x, uint32_t y) {
    const rg_scene_desc *s = f->c.s;
    int32_t bi = -1;
    double d = INFINITY;
    float n3[3] = {0.0f, 0.0f, 0.0f}, t2[2] = {0.0f, 0.0f};
    float a3[3] = {s->default_color[0], s->default_color[1], s->default_color[2]};
    pix_t px;
    memset(&px, 0, sizeof px);
    ray_t r = f->cam ? camera_ray(f, x, y) : create_prime(&f->c, x, y, f->w, f->h);
    f->total.primary++;
    if (trace(&f->c, &r, &d, &bi, &px)) {
        const rg_body *b = &s->bodies[bi];
        v3 hit = v3_add(r.o, v3_scale(r.d, d)); /* rendering.rs get_color */
        if (f->normal) {
            v3 n;
            if (!surface_normal(b, hit, &n)) {
                if (!px.err) px.err = RG_ERR_AABB_NORMAL;
                n = v3_make(1.0, 0.0, 0.0);
            }
            n3[0] = (float)n.x; n3[1] = (float)n.y; n3[2] = (float)n.z;
        }
        tc_t tc = texture_coords(b, hit);
        t2[0] = tc.x; t2[1] = tc.y;
        col cc = material_color(&f->c, &b->material, tc);
        a3[0] = cc.r; a3[1] = cc.g; a3[2] = cc.b;
    } else {
        bi = -1;
        d = INFINITY;
    }
    note_error(f, x, y, &px);
    aov_store(f, o, bi, d, n3, t2, a3);
}

/* Layers as in include/raingun.h (rg_aov), each nullable; `cam` nullable (create_prime). */
int32_t rga_render(const rg_scene_desc *s, uint32_t w, uint32_t h, const rg_tiling *tiling, const rg_camera *cam,
                   int32_t *body, double *depth, float *normal, float *uv, float *albedo, rg_ray_counts *counts,
                   int64_t *error_pixel) {
    rg_tiling whole = {h, 1, 0};
    if (!tiling) tiling = &whole;
    int32_t st = frame_check(s, body || depth || normal || uv || albedo, w, h, tiling);
    if (st != RG_OK) return st;
    frame_t f;
    frame_init(&f, s, w, h, cam);
    f.body = body; f.depth = depth; f.normal = normal; f.uv = uv; f.albedo = albedo;
    return walk_frame(&f, tiling, aov_pixel, aov_padding, counts, error_pixel);
}
