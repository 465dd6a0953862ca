// rg_render_heavy_d64.hip — the heavy-path kernels, 64 array frames: the one translation unit
// that emits these rg_render_kernel instantiations (rg_render_launch.h).
#include "rg_render_launch.h"

template hipError_t launch_heavy<64, false>(const RgKernelArgs *, hipStream_t, size_t *);
