// rg_render_light_d0.hip — the light-path kernels, frames in the global buffer (MAXD = 0): the one translation unit
// that emits these rg_render_kernel instantiations (rg_render_launch.h).
#include "rg_render_launch.h"

template hipError_t launch_light<0>(const RgKernelArgs *, hipStream_t, size_t *, int *);
