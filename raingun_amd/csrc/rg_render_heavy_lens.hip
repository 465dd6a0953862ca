// rg_render_heavy_lens.hip — the heavy-path kernels of lens launches (rg_scene_set_lens; the bands of a supersampled
// frame whose primary rays leave the lens disk, frames in the global buffer: MAXD = RG_MAXD_LENS): the one translation
// unit that emits these rg_render_kernel instantiations (rg_render_launch.h).
#include "rg_lens_launch.h"

template hipError_t launch_heavy<RG_MAXD_LENS, false>(const RgKernelArgs *, hipStream_t, size_t *);
