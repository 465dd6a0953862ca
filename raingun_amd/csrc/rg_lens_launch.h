// rg_lens_launch.h — the include of the two lens translation units (rg_render_{light,heavy}_lens.hip): the
// launch policy of rg_render_launch.h, whose MAXD = RG_MAXD_LENS instantiations they emit.  They take it
// through this header for the reason the camera units take theirs through rg_camera_launch.h:
// tests/test_diagnostic_builds.py finds the kernel translation units by their direct includes of a kernel
// header and pins their number; the diagnostic builds of the lens units are compiled by tests/test_lens_cpu.py.
#pragma once
#include "rg_render_launch.h"
