#!/usr/bin/env python3
"""Measure the thin lens on the GPU (separate from bench.py; DESIGN.md 4w quotes the numbers).

Every time from HIP events on the stream the work runs on, after warm-up, the compared frames
alternating in one process, the median of the timed batches reported.

The frame: 1920x1080 output pixels, 4 x 4 samples each, depth 5, device-resident (rg_render_aa_async
without stats), of test1 and of the north-star scene (1024 spheres).  Rendered three ways:

  lens      a lens of aperture 2.0 (about 2 % of the scenes' extent of ~100) focused on the scene's centre:
            the lens family, rays spread over the lens disk;
  pinpoint  the same lens with aperture 1e-9: the lens family and all of its arithmetic at the RGR_PRIM
            site, but rays that leave (to 1e-9) one point, as coherent as the camera's;
  camera    the identity camera and no lens: the camera family -- the same kernels minus the lens site,
            the same rays minus their spread.

lens / camera is the price of depth of field; pinpoint / camera isolates the lens site's ALU and table
loads, lens / pinpoint what the spread of the primary rays costs the walk and everything behind it.

Writes one JSON document (default profiles/lens/lens_bench.json).
"""
from __future__ import annotations

import argparse
import statistics
import sys

import rg_measure as rm
from rg_measure import REPO, summary


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(REPO / "profiles" / "lens" / "lens_bench.json"))
    rm.add_timing_args(ap, batches=7, per_batch=10, warmup=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=4)
    args = ap.parse_args(argv)

    import torch

    from raingun_amd import _abi
    from raingun_amd.camera import Camera, Lens
    from raingun_amd.scene import DeviceScene

    rm.require_gpu("lens_bench.py")
    stream = torch.cuda.Stream()
    W, H, K = args.width, args.height, args.samples

    result = {**rm.header(args, W, H), "samples": K, "max_depth": 5, "scenes": {}}
    focus_of = {"test1": 30.0, "north_star_1024_spheres": 49.0}  # distance of the scene's centre down -z: the plane in focus
    bufs = {v: torch.empty((H, W, 4), dtype=torch.uint8, device="cuda") for v in ("lens", "pinpoint", "camera")}

    for name, scene in rm.bench_scenes().items():
        focus = focus_of[name]
        variants = {"lens": Lens(2.0, focus), "pinpoint": Lens(1e-9, focus), "camera": None}
        dss, la = {}, {}
        for v, lens in variants.items():
            ds = DeviceScene(scene)
            ds.set_camera(Camera.identity())
            ds.set_lens(lens)
            dss[v], la[v] = ds, rm.Launches(ds, W, H, stream)

        stats = {v: _abi.rg_stats() for v in variants}
        for v in variants:
            la[v].aa(K, bufs[v], stats=stats[v])
        differ = int((bufs["lens"] != bufs["camera"]).any(dim=2).sum().item())
        assert differ > 0, "the lens changed no pixel"
        r = rm.alternate({v: (lambda v=v: la[v].aa(K, bufs[v])) for v in variants},
                         rm.event_batch_ms(stream, args.per_batch), args.warmup, args.batches)
        med = {v: statistics.median(r[v]) for v in variants}
        result["scenes"][name] = {
            "aperture": 2.0, "focus": focus, "pixels_that_differ_from_the_pinhole": differ,
            "rays": {v: stats[v].rays.as_dict() for v in variants},
            "lens": summary(r["lens"]), "pinpoint": summary(r["pinpoint"]), "camera": summary(r["camera"]),
            "lens_over_camera": med["lens"] / med["camera"],
            "pinpoint_over_camera": med["pinpoint"] / med["camera"],
            "lens_over_pinpoint": med["lens"] / med["pinpoint"],
        }
        for ds in dss.values():
            ds.close()

    rm.write_record(result, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
