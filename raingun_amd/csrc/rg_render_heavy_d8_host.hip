// rg_render_heavy_d8_host.hip — the heavy-path kernels, 8 array frames, host-frame features (HF): the one translation unit
// that emits these rg_render_kernel instantiations (rg_render_launch.h).
#include "rg_render_launch.h"

template hipError_t launch_heavy<8, true>(const RgKernelArgs *, hipStream_t, size_t *);
