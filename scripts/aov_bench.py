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
import statistics
import sys

import rg_measure as rm
from rg_measure import REPO, summary


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(REPO / "profiles" / "aov" / "aov_bench.json"))
    ap.add_argument("--label", default="default build")
    rm.add_timing_args(ap, batches=7, per_batch=10, warmup=3)
    ap.add_argument("--aov-only", action="store_true", help="skip the beauty frames (A/B runs of the AOV kernel)")
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    from raingun_amd import _abi, aov
    from raingun_amd.camera import Camera
    from raingun_amd.scene import DeviceScene

    rm.require_gpu("aov_bench.py")
    stream = torch.cuda.Stream()
    W, H = 3840, 2160
    batch_ms = rm.event_batch_ms(stream, args.per_batch)
    result = {**rm.header(args, W, H), "bytes_per_pixel": {"all": 44, "body_depth": 12}, "scenes": {}}
    scenes = rm.bench_scenes()
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
                la = rm.Launches(ds, W, H, stream)
                st = _abi.rg_stats()
                la.aov(v_all, st)
                assert st.rays.as_dict() == {"primary": W * H, "shadow": 0, "secondary": 0}, st.rays.as_dict()
                host = ds.render_aov(W, H, ("body", "depth", "normal", "albedo"))
                for n, a in host.items():  # the device-resident launch against the blocking entry point
                    assert np.array_equal(layers[n].cpu().numpy().view(np.uint8), a.view(np.uint8)), n
                fns = {"aov_all": lambda: la.aov(v_all), "aov_body_depth": lambda: la.aov(v_bd),
                       "fill_44B_per_pixel": lambda: fill_all.fill_(1), "fill_12B_per_pixel": lambda: fill_bd.fill_(1)}
                if not args.aov_only:
                    fns["frame_depth5"] = lambda: la.frame(rgba)
                r = rm.alternate(fns, batch_ms, args.warmup, args.batches)
                assert ds.stream_status(stream.cuda_stream) == (0, -1)
                med = {k: statistics.median(x) for k, x in r.items()}
                row = {k: summary(x) for k, x in r.items()}
                row["hit_fraction"] = float((layers["body"] >= 0).float().mean().item())
                row["aov_all_over_store_floor"] = med["aov_all"] / med["fill_44B_per_pixel"]
                row["aov_body_depth_over_store_floor"] = med["aov_body_depth"] / med["fill_12B_per_pixel"]
                row["aov_all_GBps"] = W * H * 44 / med["aov_all"] / 1e6
                if not args.aov_only:
                    row["aov_all_over_frame"] = med["aov_all"] / med["frame_depth5"]
                    row["aov_body_depth_over_frame"] = med["aov_body_depth"] / med["frame_depth5"]
                result["scenes"][name][view] = row
                ds.close()

    rm.write_record(result, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
