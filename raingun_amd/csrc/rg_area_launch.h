// rg_area_launch.h — the include of the two area translation units (rg_render_{light,heavy}_area.hip): the
// launch policy of rg_render_launch.h, whose MAXD = RG_MAXD_AREA instantiations they emit.  They take it
// through this header for the reason the lens units take theirs through rg_lens_launch.h:
// tests/test_diagnostic_builds.py finds the kernel translation units by their direct includes of a kernel
// header and pins their number; the diagnostic builds of the area units are compiled by tests/test_area_cpu.py.
#pragma once
#include "rg_render_launch.h"
