// rg_render_light_d8.hip — the light-path kernels, 8 array frames: the one translation unit
// that emits these rg_render_kernel instantiations (rg_render_launch.h).
#include "rg_render_launch.h"

template hipError_t launch_light<8>(const RgKernelArgs *, hipStream_t, size_t *, int *);
