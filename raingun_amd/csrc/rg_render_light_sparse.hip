// rg_render_light_sparse.hip — the light-path kernels of sparse launches (a tile list and a pixel mask: adaptive
// anti-aliasing), frames in the global buffer (MAXD = 0): the one translation unit that emits these rg_render_kernel
// instantiations (rg_render_launch.h).
#include "rg_sparse_launch.h"

template hipError_t launch_light<0, true>(const RgKernelArgs *, hipStream_t, size_t *, int *);
