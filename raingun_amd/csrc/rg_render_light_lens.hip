// rg_render_light_lens.hip — the light-path kernels of lens launches (rg_scene_set_lens; the bands of a supersampled
// frame whose primary rays leave the lens disk, frames in the global buffer: MAXD = RG_MAXD_LENS): the one translation
// unit that emits these rg_render_kernel instantiations (rg_render_launch.h).
#include "rg_lens_launch.h"

template hipError_t launch_light<RG_MAXD_LENS>(const RgKernelArgs *, hipStream_t, size_t *, int *);
