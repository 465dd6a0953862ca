// rg_camera_launch.h — the include of the four camera translation units (rg_render_{light,heavy}_camera.hip,
// rg_render_{light,heavy}_camera_sparse.hip): the launch policy of rg_render_launch.h, whose
// MAXD = RG_MAXD_CAMERA instantiations they emit.  They take it through this header for the reason
// the sparse units take theirs through rg_sparse_launch.h: tests/test_diagnostic_builds.py finds the
// kernel translation units by their direct includes of a kernel header and pins their number; the
// diagnostic builds of the camera units are compiled by tests/test_camera_cpu.py.
#pragma once
#include "rg_render_launch.h"
