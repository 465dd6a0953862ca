/* ao_ref.c — the reference for the ambient occlusion pass (tests/ao_ref.py builds and loads it; nothing in
 * raingun_amd/ may).  This file includes tests/native/ref_frames.c unchanged -- the oracle, the pixel loop, the
 * camera ray -- and adds ONE entry, rgao_render: rga_render's pixel loop and primary ray, the oracle's
 * surface_normal, the oracle's trace (with its NaN rule) for every AO ray, and steps 3-8 of the contract
 * (include/raingun.h, rg_ao), written from the contract's text, independently of raingun_amd/csrc/rg_ao.h.
 * The two tables (rg_ao_tables' points, rg_lens_tables' rotations) are the caller's: no transcendental is
 * evaluated here.  tests/test_ao_cpu.py ties it to rgo_trace through a numpy restatement of the rays.
 * One thread, as ref_frames.c. */
#include "ref_frames.c"

typedef struct {
    frame_t f; /* first: the pixel callbacks take the frame */
    uint32_t k;
    double radius, bias;
    const double *ao_points, *turns;
    float *ao;
    int32_t *open_out; /* nullable: rays not occluded, -1 on a miss and in padding rows */
    double *rays_out;  /* nullable: per output pixel k^2 rays {origin, direction}, zeros where none is traced */
} ao_frame_t;

static void ao_padding(frame_t *f, size_t o) {
    ao_frame_t *A = (ao_frame_t *)f;
    A->ao[o] = 0.0f;
    if (A->open_out) A->open_out[o] = -1;
}

static void ao_pixel(frame_t *f, size_t o, uint32_t x, uint32_t y) {
    ao_frame_t *A = (ao_frame_t *)f;
    const rg_scene_desc *s = f->c.s;
    const uint32_t k2 = A->k * A->k;
    pix_t px;
    memset(&px, 0, sizeof px);
    /* 1. the primary ray */
    ray_t r = f->cam ? camera_ray(f, x, y) : create_prime(&f->c, x, y, f->w, f->h);
    double t;
    int32_t bi;
    f->total.primary++;
    if (!trace(&f->c, &r, &t, &bi, &px)) {
        note_error(f, x, y, &px);
        A->ao[o] = 1.0f;
        if (A->open_out) A->open_out[o] = -1;
        return;
    }
    /* 2. hit point and normal */
    v3 h = v3_add(r.o, v3_scale(r.d, t));
    v3 n;
    if (!surface_normal(&s->bodies[bi], h, &n)) {
        if (!px.err) px.err = RG_ERR_AABB_NORMAL;
        n = v3_make(1.0, 0.0, 0.0);
    }
    /* 3. the facing normal */
    v3 m = v3_normalize(n);
    v3 nf = v3_dot(m, r.d) <= 0.0 ? m : v3_neg(m);
    /* 4. the origin */
    v3 O = v3_make(h.x + nf.x * A->bias, h.y + nf.y * A->bias, h.z + nf.z * A->bias);
    /* 5. the tangent frame */
    double sg = copysign(1.0, nf.z);
    double a = -1.0 / (sg + nf.z);
    double b = (nf.x * nf.y) * a;
    v3 T = v3_make(1.0 + (sg * nf.x) * (nf.x * a), sg * b, (-sg) * nf.x);
    v3 B = v3_make(b, sg + (nf.y * nf.y) * a, -nf.y);
    /* 6. the pixel's turn */
    uint32_t p = y * f->w + x;
    uint32_t hsh = lowbias32(p);
    double c = A->turns[2 * (hsh & 63u)], g = A->turns[2 * (hsh & 63u) + 1];
    v3 Tr = v3_make(c * T.x + g * B.x, c * T.y + g * B.y, c * T.z + g * B.z);
    v3 Br = v3_make(c * B.x - g * T.x, c * B.y - g * T.y, c * B.z - g * T.z);
    /* 7. the sample rays */
    uint32_t open = 0;
    for (uint32_t j = 0; j < k2; ++j) {
        double qx = A->ao_points[3 * j], qy = A->ao_points[3 * j + 1], qz = A->ao_points[3 * j + 2];
        v3 D = v3_make((Tr.x * qx + Br.x * qy) + nf.x * qz, (Tr.y * qx + Br.y * qy) + nf.y * qz,
                       (Tr.z * qx + Br.z * qy) + nf.z * qz);
        ray_t q = ray_new(O, v3_normalize(D));
        if (A->rays_out) {
            double *w = A->rays_out + 6 * ((size_t)o * k2 + j);
            w[0] = q.o.x; w[1] = q.o.y; w[2] = q.o.z; w[3] = q.d.x; w[4] = q.d.y; w[5] = q.d.z;
        }
        double qt;
        int32_t qb;
        f->total.shadow++;
        int occluded = trace(&f->c, &q, &qt, &qb, &px) && !(qt > A->radius); /* rendering.rs:150-155 */
        if (!occluded) open++;
    }
    note_error(f, x, y, &px);
    /* 8. the value */
    A->ao[o] = (float)open / (float)k2;
    if (A->open_out) A->open_out[o] = (int32_t)open;
}

/* `cam` nullable (create_prime); ao: rgo_tiling_rows x w floats; ao_points: 3 k^2 doubles; turns: 128 doubles;
 * open_out (rows x w) and rays_out (rows x w x k^2 x 6, zeroed by the caller) nullable. */
int32_t rgao_render(const rg_scene_desc *s, uint32_t w, uint32_t h, const rg_tiling *tiling, const rg_camera *cam,
                    uint32_t k, double radius, double bias, const double *ao_points, const double *turns, float *ao,
                    int32_t *open_out, double *rays_out, rg_ray_counts *counts, int64_t *error_pixel) {
    rg_tiling whole = {h, 1, 0};
    if (!tiling) tiling = &whole;
    int entry_ok = ao && ao_points && turns && k >= 1 && k <= 8 && radius > 0.0 && bias >= 0.0 && bias - bias == 0.0;
    int32_t st = frame_check(s, entry_ok, w, h, tiling);
    if (st != RG_OK) return st;
    ao_frame_t A;
    frame_init(&A.f, s, w, h, cam);
    A.k = k; A.radius = radius; A.bias = bias;
    A.ao_points = ao_points; A.turns = turns;
    A.ao = ao; A.open_out = open_out; A.rays_out = rays_out;
    return walk_frame(&A.f, tiling, ao_pixel, ao_padding, counts, error_pixel);
}
