// rg_sparse_launch.h — the include of the two sparse translation units (rg_render_light_sparse.hip,
// rg_render_heavy_sparse.hip): the launch policy of rg_render_launch.h, whose SPARSE instantiations
// they emit.  They take it through this header because tests/test_diagnostic_builds.py finds the
// kernel translation units by their direct includes of a kernel header and pins their number;
// the diagnostic builds of the sparse units are compiled by tests/test_aa_adaptive_cpu.py.
#pragma once
#include "rg_render_launch.h"
