/* area_ref.c — the reference for frames with area lights (tests/area_ref.py builds and loads it; nothing in
 * raingun_amd/ may).  The offset of a light does not depend on the hit, so the colour of sample (X, Y) is the
 * pinned oracle's colour of that sample's primary ray in a copy of the scene whose spherical lights sit at
 * `position` (include/raingun.h, rg_scene_set_light_radii).  This file includes tests/native/ref_frames.c
 * unchanged -- the oracle, the pixel loop, the camera ray and the lens ray -- and adds ONE entry, rgar_render:
 * per sample it moves the lights in a copy of the light array and calls the existing colour path
 * (camera_pixel, or lens_pixel where aperture > 0).  No shading arithmetic is restated; the index and offset
 * rule is, from the contract's text, independently of raingun_amd/csrc/rg_area.h.
 * tests/test_area_cpu.py ties it to rgl_render / rgc_render (every radius 0: their bits).
 * One thread, as ref_frames.c: the copy of the light array is the frame's. */
#include <stdlib.h>

#include "ref_frames.c"

typedef struct {
    frame_t f; /* first: the pixel callbacks take the frame */
    const rg_light *centre;
    rg_light *moved;
    rg_scene_desc copy;
    const double *radii, *sphere_points;
    uint32_t out_w;
    int through_lens;
} area_frame_t;

static void area_pixel(frame_t *f, size_t o, uint32_t x, uint32_t y) {
    area_frame_t *A = (area_frame_t *)f;
    const uint32_t k = f->k;
    const uint32_t sidx = (y % k) * k + (x % k);
    const uint32_t n = (y / k) * A->out_w + (x / k);
    for (uint32_t l = 0; l < A->copy.n_lights; ++l) {
        if (A->centre[l].kind != RG_LIGHT_SPHERICAL) continue;
        const uint32_t g = lowbias32(n ^ ((l + 1u) * 0x9e3779b9u));
        const uint32_t j = (sidx + (g >> 6)) % (k * k);
        const double c = f->rotations[2 * (g & 63u)], e = f->rotations[2 * (g & 63u) + 1];
        const double px = A->sphere_points[3 * j], py = A->sphere_points[3 * j + 1], pz = A->sphere_points[3 * j + 2];
        const double qx = c * px - e * py, qy = e * px + c * py, qz = pz;
        A->moved[l].v[0] = A->centre[l].v[0] + A->radii[l] * qx;
        A->moved[l].v[1] = A->centre[l].v[1] + A->radii[l] * qy;
        A->moved[l].v[2] = A->centre[l].v[2] + A->radii[l] * qz;
    }
    if (A->through_lens) lens_pixel(f, o, x, y);
    else camera_pixel(f, o, x, y);
}

/* w, h: the OUTPUT frame; k x k samples per pixel; rgba / rgb: the (k h) x (k w) sample frame, walked whole.
 * aperture > 0: through the lens {aperture, focus} (lens_points: 2 k^2 doubles), else the camera ray.
 * rotations: 128 doubles; sphere_points: 3 k^2 doubles; radii: one per light of the scene. */
int32_t rgar_render(const rg_scene_desc *s, uint32_t w, uint32_t h, uint32_t k, const rg_camera *cam, double aperture,
                    double focus, const double *lens_points, const double *rotations, const double *sphere_points,
                    const double *radii, uint8_t *rgba, float *rgb, rg_ray_counts *counts, int64_t *error_pixel) {
    const rg_tiling whole = {k * h, 1, 0};
    int32_t st = frame_check(s, rgba && cam && lens_points && rotations && sphere_points && (radii || s->n_lights == 0) && k != 0,
                             w, h, &whole);
    if (st != RG_OK) return st;
    area_frame_t A;
    frame_init(&A.f, s, k * w, k * h, cam);
    A.f.rgba = rgba; A.f.rgb = rgb;
    A.f.k = k; A.f.focus = focus; A.f.points = lens_points; A.f.rotations = rotations;
    A.f.LR = lens_axis(A.f.right, aperture); A.f.LU = lens_axis(A.f.up, aperture);
    A.centre = s->lights;
    A.moved = malloc((s->n_lights ? s->n_lights : 1) * sizeof *A.moved);
    if (!A.moved) return RG_ERR_OUT_OF_MEMORY;
    if (s->n_lights) memcpy(A.moved, s->lights, s->n_lights * sizeof *A.moved);
    A.copy = *s;
    A.copy.lights = A.moved;
    A.f.c.s = &A.copy; /* every sample is traced in the copy */
    A.radii = radii; A.sphere_points = sphere_points; A.out_w = w;
    A.through_lens = aperture > 0.0;
    st = walk_frame(&A.f, &whole, area_pixel, colour_padding, counts, error_pixel);
    free(A.moved);
    return st;
}
