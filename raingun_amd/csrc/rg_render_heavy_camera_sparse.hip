// rg_render_heavy_camera_sparse.hip — the heavy-path kernels of camera launches that are sparse (a tile list and a pixel mask) (rg_scene_set_camera; primary rays from the
// camera's eye, frames in the global buffer: MAXD = RG_MAXD_CAMERA): the one translation unit that emits these
// rg_render_kernel instantiations (rg_render_launch.h).
#include "rg_camera_launch.h"

template hipError_t launch_heavy<RG_MAXD_CAMERA, false, true>(const RgKernelArgs *, hipStream_t, size_t *);
