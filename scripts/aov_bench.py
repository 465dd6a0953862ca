#!/usr/bin/env python3
"""Measure the AOV layers on the GPU (separate from bench.py; DESIGN.md 4u quotes the numbers).

Every time from HIP events on the stream the work runs on, after warm-up, the compared launches
alternating in one process, the median of the timed batches reported.  test1 (depth 5) and the
north-star scene (1024 spheres, depth 5) at 3840x2160, device-resident single launches, under the fixed
view and under the IDENTITY camera (the same rays through the general closest-hit query):

(i)   rg_render_aov_async, all five layers (44 B per pixel: 365 MB);
(ii)  rg_render_aov_async, body + depth only (12 B per pixel): the trace alone;
(iii) the same scene's rg_render_tiles_async frame at depth 5, the yardstick: (i) traces a strict subset
      of its rays.

Beside them the store floor: the time the device takes to write as many bytes as (i) and (ii) store
(a fill of one buffer of that size, same stream, same alternation).  (i) / floor says whether the store
layout or the trace bounds the kernel.  The layers are compared with the blocking entry point's first.

Writes one JSON document (default profiles/aov/aov_bench.json).  RAINGUN_HIP_LIB selects another build
of the library (A/B runs of the lane-to-pixel mapping, RG_AOV_TILE_WLOG); --label names it in the JSON.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def _summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "batches": len(ms)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(REPO / "profiles" / "aov" / "aov_bench.json"))
    ap.add_argument("--label", default="default build")
    ap.add_argument("--batches", type=int, default=7, help="timed batches per variant (the median is reported)")
    ap.add_argument("--per-batch", type=int, default=10, help="launches per timed batch")
    ap.add_argument("--warmup", type=int, default=3, help="untimed batches first")
    ap.add_argument("--aov-only", action="store_true", help="skip the beauty frames (A/B runs of the AOV kernel)")
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    from raingun_amd import _abi, aov
    from raingun_amd.camera import Camera
    from raingun_amd.scene import DeviceScene, load_scene
    from raingun_amd.synth import synthetic_scene

    if not torch.cuda.is_available():
        raise SystemExit("aov_bench.py needs a GPU: nothing is measured without one")
    lib = _abi.lib()
    stream = torch.cuda.Stream()
    hs = C.c_void_p(stream.cuda_stream)
    W, H = 3840, 2160
    whole = _abi.rg_tiling(H, 1, 0)

    def batch_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.per_batch):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.per_batch

    def alternate(fns):
        for fn in fns.values():
            for _ in range(args.warmup):
                batch_ms(fn)
        res = {k: [] for k in fns}
        for _ in range(args.batches):
            for k, fn in fns.items():
                res[k].append(batch_ms(fn))
        return res

    result = {"device": torch.cuda.get_device_name(0), "library": os.environ.get("RAINGUN_HIP_LIB", "raingun_amd/libraingun_hip.so"),
              "label": args.label, "per_batch": args.per_batch, "batches": args.batches, "width": W, "height": H,
              "bytes_per_pixel": {"all": 44, "body_depth": 12}, "scenes": {}}
    golden = REPO / "tests" / "golden"
    test1 = load_scene(golden / "examples" / "test1.yml", texture_root=golden)
    test1.max_recursion_depth = 5
    scenes = {"test1": test1, "north_star_1024_spheres": synthetic_scene(1024, 2, 5)}
    tt = {np.int32: torch.int32, np.float64: torch.float64, np.float32: torch.float32}
    layers = {n: torch.empty(aov.layer_shape(n, H, W), dtype=tt[aov.DTYPES[n]], device="cuda") for n in aov.LAYERS}
    rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    fill_all = torch.empty((W * H * 44,), dtype=torch.uint8, device="cuda")
    fill_bd = torch.empty((W * H * 12,), dtype=torch.uint8, device="cuda")
    v_all = _abi.rg_aov(**{n: t.data_ptr() for n, t in layers.items()})
    v_bd = _abi.rg_aov(body=layers["body"].data_ptr(), depth=layers["depth"].data_ptr())

    with torch.cuda.stream(stream):
        for name, scene in scenes.items():
            result["scenes"][name] = {}
            for view, cam in (("fixed_view", None), ("identity_camera", Camera.identity())):
                ds = DeviceScene(scene)
                ds.set_camera(cam)

                def launch_aov(v, stats=None):
                    _abi.check(lib.rg_render_aov_async(ds.handle, W, H, C.byref(whole), C.byref(v), hs,
                                                       C.byref(stats) if stats is not None else None))

                def launch_frame():
                    _abi.check(lib.rg_render_tiles_async(ds.handle, W, H, C.byref(whole), C.c_void_p(rgba.data_ptr()), None,
                                                         hs, None))

                st = _abi.rg_stats()
                launch_aov(v_all, st)
                assert st.rays.as_dict() == {"primary": W * H, "shadow": 0, "secondary": 0}, st.rays.as_dict()
                host = ds.render_aov(W, H, ("body", "depth", "normal", "albedo"))
                for n, a in host.items():  # the device-resident launch against the blocking entry point
                    assert np.array_equal(layers[n].cpu().numpy().view(np.uint8), a.view(np.uint8)), n
                fns = {"aov_all": lambda: launch_aov(v_all), "aov_body_depth": lambda: launch_aov(v_bd),
                       "fill_44B_per_pixel": lambda: fill_all.fill_(1), "fill_12B_per_pixel": lambda: fill_bd.fill_(1)}
                if not args.aov_only:
                    fns["frame_depth5"] = launch_frame
                r = alternate(fns)
                assert ds.stream_status(stream.cuda_stream) == (0, -1)
                med = {k: statistics.median(x) for k, x in r.items()}
                row = {k: _summary(x) for k, x in r.items()}
                row["hit_fraction"] = float((layers["body"] >= 0).float().mean().item())
                row["aov_all_over_store_floor"] = med["aov_all"] / med["fill_44B_per_pixel"]
                row["aov_body_depth_over_store_floor"] = med["aov_body_depth"] / med["fill_12B_per_pixel"]
                row["aov_all_GBps"] = W * H * 44 / med["aov_all"] / 1e6
                if not args.aov_only:
                    row["aov_all_over_frame"] = med["aov_all"] / med["frame_depth5"]
                    row["aov_body_depth_over_frame"] = med["aov_body_depth"] / med["frame_depth5"]
                result["scenes"][name][view] = row
                ds.close()

    outp = Path(args.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
