"""What the feature benchmarks under scripts/ share: the measuring loop (warm-up, timed batches between two HIP
events on the stream the work runs on, the variants alternating in one process, median with spread), the scene
set, the record's header and tail, and the device-resident launches they time.

A plain module beside the scripts (`import rg_measure`): torch and the package are imported inside the
functions that need them, so it imports without a GPU.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "batches": len(ms)}


def event_batch_ms(stream, per_batch):
    """-> batch_ms(fn): the HIP-event time of per_batch calls of fn on `stream`, per call."""
    import torch

    def batch_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(per_batch):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / per_batch

    return batch_ms


def alternate(fns, batch_ms, warmup, batches):
    """Each of fns warmed up (`warmup` untimed batches), then timed `batches` times, one batch of each in turn
    -> {name: [ms, ...]}."""
    for fn in fns.values():
        for _ in range(warmup):
            batch_ms(fn)
    res = {k: [] for k in fns}
    for _ in range(batches):
        for k, fn in fns.items():
            res[k].append(batch_ms(fn))
    return res


def add_timing_args(ap, batches, per_batch, warmup):
    """--batches / --per-batch / --warmup with the calling script's own defaults."""
    ap.add_argument("--batches", type=int, default=batches, help="timed batches per variant (the median is reported)")
    ap.add_argument("--per-batch", type=int, default=per_batch, help="launches or frames per timed batch")
    ap.add_argument("--warmup", type=int, default=warmup, help="untimed batches first")


def require_gpu(script):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit(f"{script} needs a GPU: nothing is measured without one")


def golden():
    return REPO / "tests" / "golden"


def bench_scenes():
    """test1 at depth 5 and the north-star scene of bench.py (1024 spheres + 2 planes, depth 5)."""
    from raingun_amd.scene import load_scene
    from raingun_amd.synth import synthetic_scene

    test1 = load_scene(golden() / "examples" / "test1.yml", texture_root=golden())
    test1.max_recursion_depth = 5
    return {"test1": test1, "north_star_1024_spheres": synthetic_scene(1024, 2, 5)}


def header(args, width=None, height=None):
    """The record's common keys (width and height left out by a script whose sections have sizes of their own)."""
    import torch

    h = {"device": torch.cuda.get_device_name(0),
         "library": os.environ.get("RAINGUN_HIP_LIB", "raingun_amd/libraingun_hip.so"),
         "label": getattr(args, "label", "default build"), "per_batch": args.per_batch, "batches": args.batches}
    if width is not None:
        h.update(width=width, height=height)
    return h


def write_record(result, out, echo=True):
    """The JSON document into `out` (if given) and, with echo, on stdout as one line."""
    if out:
        outp = Path(out)
        outp.parent.mkdir(parents=True, exist_ok=True)
        outp.write_text(json.dumps(result, indent=1) + "\n")
    if echo:
        print(json.dumps(result))


def ab_table(ab):
    """The lines of an A/B record's table: one row per build, one column per measured case, median ms."""
    cols = sorted({s for v in ab.values() for s in v})
    lines = ["| build | " + " | ".join(cols) + " |", "|---|" + "---|" * len(cols)]
    for key, v in ab.items():
        lines.append(f"| {key} | " + " | ".join(f"{v[s]['median_ms']:.3f}" if s in v else "" for s in cols) + " |")
    return lines + [""]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _ref(s):
    return C.byref(s) if s is not None else None


class Launches:
    """The device-resident whole-frame launches of one scene at one size on one stream."""

    def __init__(self, ds, width, height, stream):
        from raingun_amd import _abi

        self._abi, self.lib, self.ds, self.w, self.h = _abi, _abi.lib(), ds, width, height
        self.whole = _abi.rg_tiling(height, 1, 0)
        self.hs = C.c_void_p(stream.cuda_stream)

    def frame(self, rgba, rgb=None, stats=None):
        self._abi.check(self.lib.rg_render_tiles_async(self.ds.handle, self.w, self.h, C.byref(self.whole), _p(rgba),
                                                       _p(rgb), self.hs, _ref(stats)), "rg_render_tiles_async")

    def aa(self, k, rgba, rgb=None, stats=None):
        self._abi.check(self.lib.rg_render_aa_async(self.ds.handle, self.w, self.h, k, _p(rgba), _p(rgb), self.hs,
                                                    _ref(stats)), "rg_render_aa_async")

    def aov(self, v, stats=None):
        self._abi.check(self.lib.rg_render_aov_async(self.ds.handle, self.w, self.h, C.byref(self.whole), C.byref(v),
                                                     self.hs, _ref(stats)), "rg_render_aov_async")

    def ao(self, v, out, stats=None):
        self._abi.check(self.lib.rg_render_ao_async(self.ds.handle, self.w, self.h, C.byref(self.whole), C.byref(v),
                                                    _p(out), self.hs, _ref(stats)), "rg_render_ao_async")
