"""The render kernel's diagnostic builds still compile (CPU, no GPU needed).

The kernel headers (rg_render_kernel.h, rg_k_*.h) keep default-off diagnostic
switches (per-tile and per-wave timelines, per-iteration SIMD-use counters, BVH
statistics, region visit counts) that scripts under scripts/ build into variant
libraries for profiling sessions.  Every other default-off experiment was
removed; these must not rot, so each one is compiled here (hipcc
semantic analysis of every translation unit that includes a kernel header,
every template instantiation included, for gfx950)."""
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "raingun_amd" / "csrc"
HIPCC = "/opt/rocm/bin/hipcc"
# every translation unit that includes a kernel header directly: nine of the eleven rg_render_*.hip
# (one group of rg_render_kernel instantiations each; the two sparse ones take theirs through
# rg_sparse_launch.h and are compiled by tests/test_aa_adaptive_cpu.py), the launchers with
# rg_trace_kernel, the tile-order kernels: eleven units
KERNEL_UNITS = sorted(p.name for p in CSRC.glob("*.hip")
                      if any(h in p.read_text() for h in ('#include "rg_k_', '#include "rg_render_')))


@pytest.mark.skipif(shutil.which(HIPCC) is None and not Path(HIPCC).exists(), reason="hipcc not installed")
@pytest.mark.parametrize("flag", ["", "-DRG_TILE_TIMES", "-DRG_WAVE_TIMES", "-DRG_ITER_STATS", "-DRG_BVH_STATS",
                                  "-DRG_REGION_STATS"])
def test_diagnostic_build_compiles(flag):
    assert len(KERNEL_UNITS) == 11, KERNEL_UNITS
    cmd = [HIPCC, "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fsyntax-only", "-Werror=return-type"]
    if flag:
        cmd.append(flag)
    procs = [(u, subprocess.Popen(cmd + [u], cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True))
             for u in KERNEL_UNITS]
    results = [(u, p, p.communicate(timeout=600)[1]) for u, p in procs]
    for u, p, err in results:
        assert p.returncode == 0, (u, err[-3000:])
        assert " error:" not in err, (u, err[-3000:])
