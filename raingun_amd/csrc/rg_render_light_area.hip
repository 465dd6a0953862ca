// rg_render_light_area.hip — the light-path kernels of area-light launches (rg_scene_set_light_radii; the bands of a
// supersampled frame whose spherical lights are seen at a point of their sphere per sample, frames in the global
// buffer: MAXD = RG_MAXD_AREA): the one translation unit that emits these rg_render_kernel instantiations
// (rg_render_launch.h).
#include "rg_area_launch.h"

template hipError_t launch_light<RG_MAXD_AREA>(const RgKernelArgs *, hipStream_t, size_t *, int *);
