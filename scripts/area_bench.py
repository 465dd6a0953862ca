#!/usr/bin/env python3
"""Measure the area lights on the GPU (separate from bench.py; DESIGN.md 4y quotes the numbers).

Every time from HIP events on the stream the work runs on, after warm-up, the compared frames
alternating in one process, the median of the timed batches reported.

The frame: test1 at 1920x1080 output pixels, 4 x 4 samples each, depth 5, device-resident
(rg_render_aa_async without stats).  Rendered these ways:

  area       a radius on each of its spherical lights (1.0 and 5.0: about a sixth of each light's distance
             from the scene): the area family, every light at a point of its sphere per sample;
  area_lens  the same through a lens of aperture 2.0 focused on the scene's centre: the same family, lens rays;
  point      no radii, no camera, no lens: the supersampled frame as the scene rendered it before;
  parent     (with --parent-lib) that point-light frame by another build of the library -- the parent
             commit's -- loaded beside this one and interleaved with the three above.

area / point is the price of soft shadows; point / parent shows that the point-light frame kept its time
(to be read against the spread of `parent`'s own batches).

Writes one JSON document (default profiles/area/area_bench.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

import rg_measure as rm
from rg_measure import REPO, summary


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(REPO / "profiles" / "area" / "area_bench.json"))
    ap.add_argument("--parent-lib", default=None, help="a libraingun_hip.so of the parent commit, for the `parent` frame")
    rm.add_timing_args(ap, batches=7, per_batch=10, warmup=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=4)
    args = ap.parse_args(argv)

    import torch

    from raingun_amd import _abi
    from raingun_amd.camera import Lens
    from raingun_amd.scene import DeviceScene, SceneDesc, SphericalLight

    rm.require_gpu("area_bench.py")
    lib = _abi.lib()
    stream = torch.cuda.Stream()
    hs = C.c_void_p(stream.cuda_stream)
    W, H, K = args.width, args.height, args.samples

    test1 = rm.bench_scenes()["test1"]
    spherical = [isinstance(l, SphericalLight) for l in test1.lights]
    radii = [r if s else 0.0 for r, s in zip((1.0, 1.0, 5.0), spherical)]
    assert len(spherical) == 3 and sum(spherical) == 2
    variants = {"area": (radii, None), "area_lens": (radii, Lens(2.0, 30.0)), "point": (None, None)}
    bufs = {v: torch.empty((H, W, 4), dtype=torch.uint8, device="cuda") for v in (*variants, "parent")}
    dss, la = {}, {}
    for v, (r, lens) in variants.items():
        ds = DeviceScene(test1)
        ds.set_lens(lens)
        ds.set_light_radii(r)
        dss[v], la[v] = ds, rm.Launches(ds, W, H, stream)

    fns = {v: (lambda v=v: la[v].aa(K, bufs[v])) for v in variants}
    parent = None
    if args.parent_lib:  # the other build, beside this one: the three entries the frame needs
        parent = C.CDLL(str(Path(args.parent_lib).resolve()))
        for fn in ("rg_scene_create", "rg_scene_destroy", "rg_render_aa_async"):
            getattr(parent, fn).restype = getattr(lib, fn).restype
            getattr(parent, fn).argtypes = getattr(lib, fn).argtypes
        desc = SceneDesc(test1)
        handle = C.c_void_p()
        _abi.check(parent.rg_scene_create(desc.ptr(), 0, C.byref(handle)), "parent rg_scene_create")

        def launch_parent():
            _abi.check(parent.rg_render_aa_async(handle, W, H, K, C.c_void_p(bufs["parent"].data_ptr()), None, hs, None),
                       "parent rg_render_aa_async")

        fns["parent"] = launch_parent

    stats = {v: _abi.rg_stats() for v in variants}
    for v in variants:
        la[v].aa(K, bufs[v], stats=stats[v])
    if parent is not None:
        fns["parent"]()
    torch.cuda.synchronize()
    differ = int((bufs["area"] != bufs["point"]).any(dim=2).sum().item())
    assert differ > 0, "the radii changed no pixel"
    if parent is not None:
        assert bool((bufs["parent"] == bufs["point"]).all().item()), "the point-light frame is not the parent's"
    r = rm.alternate(fns, rm.event_batch_ms(stream, args.per_batch), args.warmup, args.batches)
    med = {v: statistics.median(r[v]) for v in fns}
    result = {**rm.header(args, W, H), "samples": K, "max_depth": 5, "scene": "test1", "radii": radii,
              "lens": {"aperture": 2.0, "focus": 30.0},
              "pixels_that_differ_from_the_point_lights": differ,
              "rays": {v: stats[v].rays.as_dict() for v in variants},
              **{v: summary(r[v]) for v in fns},
              "area_over_point": med["area"] / med["point"],
              "area_lens_over_point": med["area_lens"] / med["point"]}
    if parent is not None:
        result["point_over_parent"] = med["point"] / med["parent"]
        result["parent_spread"] = (max(r["parent"]) - min(r["parent"])) / med["parent"]
        parent.rg_scene_destroy(handle)
    for ds in dss.values():
        ds.close()

    rm.write_record(result, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
