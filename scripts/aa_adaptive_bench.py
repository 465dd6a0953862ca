#!/usr/bin/env python3
"""Measure adaptive anti-aliasing on the GPU (separate from bench.py).

Device-resident, 3840x2160, depth 5, for test1 and the 1024-sphere north-star scene, for
samples k in {2, 4} and thresholds T in {16, 32, 64}.  Per configuration, after warm-up, the
median over interleaved repetitions (one call of each in turn, HIP events on the caller's
stream around each call; every call ends with the stream idle) of

  (a) the 1-sample frame                 rg_render_tiles_async
  (b) the full supersampled frame        rg_render_aa_async at k
  (c) the adaptive frame                 rg_render_aa_adaptive at k, T

with the flagged share F / (W H), the ray counts of the three, and the passes of (c) from HIP
events inside the library (rg_debug_aa_adaptive_info: the 1-sample pass, the mask kernel, the
list kernel, the sparse renders and the adaptive resolves, the last two summed over the bands).
The model (c) is reported against: t(a) + share * t(b) + overheads.

Writes one JSON document (default profiles/aa/aa_adaptive_bench.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys

import rg_measure as rm
from rg_measure import REPO, summary

SCENES = {"test1": "test1", "synth1024": "north_star_1024_spheres"}  # --scenes name -> rg_measure.bench_scenes()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(REPO / "profiles" / "aa" / "aa_adaptive_bench.json"))
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--scenes", default="test1,synth1024")
    ap.add_argument("--samples", default="2,4")
    ap.add_argument("--thresholds", default="16,32,64")
    ap.add_argument("--reps", "--batches", dest="batches", type=int, default=9,
                    help="timed repetitions per variant (the median is reported)")
    ap.add_argument("--warmup", type=int, default=2, help="untimed repetitions first")
    ap.add_argument("--band-rows", type=int, default=0, help="rg_debug_set_aa_band_rows (0: automatic)")
    ap.add_argument("--full-only", action="store_true",
                    help="only (a) and (b): the figures an older build gives too (the full form did not move)")
    args = ap.parse_args(argv)
    args.per_batch = 1  # `timed` below times one call

    import torch

    from raingun_amd import _abi
    from raingun_amd.scene import DeviceScene

    rm.require_gpu("aa_adaptive_bench.py")
    lib = _abi.lib()
    adaptive = hasattr(lib, "rg_render_aa_adaptive") and not args.full_only
    W, H = args.width, args.height
    stream = torch.cuda.Stream()
    hs = C.c_void_p(stream.cuda_stream)
    scenes = rm.bench_scenes()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    result = {**rm.header(args, W, H), "max_depth": 5, "band_rows": args.band_rows, "configs": []}
    rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    mask = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    for name in args.scenes.split(","):
        if name not in SCENES:
            raise SystemExit(f"unknown scene {name}")
        ds = DeviceScene(scenes[SCENES[name]])
        la = rm.Launches(ds, W, H, stream)
        ds.set_aa_band_rows(args.band_rows)
        if adaptive:
            _abi.check(lib.rg_debug_set_aa_adaptive_timing(ds.handle, 1))
        for k in (int(v) for v in args.samples.split(",")):
            for T in (int(v) for v in args.thresholds.split(",")) if adaptive else (None,):
                st = {v: _abi.rg_stats() for v in "abc"}

                def one(stats=None):
                    la.frame(rgba, stats=stats)
                    stream.synchronize()

                def full(stats=None):
                    la.aa(k, rgba, stats=stats)
                    stream.synchronize()

                def adapt(stats=None):
                    _abi.check(lib.rg_render_aa_adaptive(ds.handle, W, H, k, T, C.c_void_p(rgba.data_ptr()), None,
                                                         C.c_void_p(mask.data_ptr()), hs,
                                                         C.byref(stats) if stats is not None else None))

                fns = {"a_one_sample": one, "b_full": full}
                if adaptive:
                    fns["c_adaptive"] = adapt
                for fn in fns.values():
                    for _ in range(args.warmup):
                        fn()
                ms = {v: [] for v in fns}
                passes = []
                for _ in range(args.batches):
                    for v, fn in fns.items():
                        ms[v].append(timed(fn))
                        if v == "c_adaptive":
                            p = (C.c_float * 5)()
                            _abi.check(lib.rg_debug_aa_adaptive_info(ds.handle, p, None, None, None))
                            passes.append(list(p))
                one(st["a"])
                full(st["b"])
                cfg = {"scene": name, "samples": k, "threshold": T,
                       "a_one_sample": summary(ms["a_one_sample"]), "b_full": summary(ms["b_full"]),
                       "rays_a": st["a"].rays.as_dict(), "rays_b": st["b"].rays.as_dict()}
                if adaptive:
                    adapt(st["c"])
                    flagged, tiles, bands = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
                    _abi.check(lib.rg_debug_aa_adaptive_info(ds.handle, None, C.byref(flagged), C.byref(tiles),
                                                             C.byref(bands)))
                    assert int(mask.sum(dtype=torch.int64).item()) == flagged.value
                    assert st["c"].rays.primary == W * H + k * k * flagged.value
                    share = flagged.value / (W * H)
                    a, b, c = (statistics.median(ms[v]) for v in ("a_one_sample", "b_full", "c_adaptive"))
                    med = [statistics.median(p[i] for p in passes) for i in range(5)]
                    cfg.update({
                        "c_adaptive": summary(ms["c_adaptive"]), "rays_c": st["c"].rays.as_dict(),
                        "flagged": flagged.value, "flagged_share": share, "listed_tiles": tiles.value,
                        "tiles_of_sample_frame": ((k * W + 7) // 8) * ((k * H + 7) // 8), "bands_launched": bands.value,
                        "passes_median_ms": dict(zip(("one_sample", "mask", "list", "sparse_renders_sum",
                                                      "adaptive_resolves_sum"), med)),
                        "c_over_b": c / b, "model_a_plus_share_b_ms": a + share * b,
                        "overheads_ms": c - (a + share * b),
                    })
                result["configs"].append(cfg)
                print(json.dumps(cfg), flush=True)
        ds.close()

    rm.write_record(result, args.out, echo=False)  # each configuration was printed as it finished
    return 0


if __name__ == "__main__":
    sys.exit(main())
