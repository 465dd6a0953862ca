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
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def _summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "batches": len(ms)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(REPO / "profiles" / "lens" / "lens_bench.json"))
    ap.add_argument("--batches", type=int, default=7, help="timed batches per variant (the median is reported)")
    ap.add_argument("--per-batch", type=int, default=10, help="frames per timed batch")
    ap.add_argument("--warmup", type=int, default=2, help="untimed batches first")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=4)
    args = ap.parse_args(argv)

    import torch

    from raingun_amd import _abi
    from raingun_amd.camera import Camera, Lens
    from raingun_amd.scene import DeviceScene, load_scene
    from raingun_amd.synth import synthetic_scene

    if not torch.cuda.is_available():
        raise SystemExit("lens_bench.py needs a GPU: nothing is measured without one")
    lib = _abi.lib()
    stream = torch.cuda.Stream()
    hs = C.c_void_p(stream.cuda_stream)
    W, H, K = args.width, args.height, args.samples

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

    result = {"device": torch.cuda.get_device_name(0), "per_batch": args.per_batch, "batches": args.batches,
              "width": W, "height": H, "samples": K, "max_depth": 5, "scenes": {}}
    golden = REPO / "tests" / "golden"
    test1 = load_scene(golden / "examples" / "test1.yml", texture_root=golden)
    test1.max_recursion_depth = 5
    # (scene, distance of its centre down -z: the plane in focus)
    scenes = {"test1": (test1, 30.0), "north_star_1024_spheres": (synthetic_scene(1024, 2, 5), 49.0)}
    bufs = {v: torch.empty((H, W, 4), dtype=torch.uint8, device="cuda") for v in ("lens", "pinpoint", "camera")}

    for name, (scene, focus) in scenes.items():
        variants = {"lens": Lens(2.0, focus), "pinpoint": Lens(1e-9, focus), "camera": None}
        dss = {}
        for v, lens in variants.items():
            ds = DeviceScene(scene)
            ds.set_camera(Camera.identity())
            ds.set_lens(lens)
            dss[v] = ds

        def launch(v, stats=None):
            _abi.check(lib.rg_render_aa_async(dss[v].handle, W, H, K, C.c_void_p(bufs[v].data_ptr()), None, hs,
                                              C.byref(stats) if stats is not None else None), "rg_render_aa_async")

        stats = {v: _abi.rg_stats() for v in variants}
        for v in variants:
            launch(v, stats[v])
        differ = int((bufs["lens"] != bufs["camera"]).any(dim=2).sum().item())
        assert differ > 0, "the lens changed no pixel"
        r = alternate({v: (lambda v=v: launch(v)) for v in variants})
        med = {v: statistics.median(r[v]) for v in variants}
        result["scenes"][name] = {
            "aperture": 2.0, "focus": focus, "pixels_that_differ_from_the_pinhole": differ,
            "rays": {v: stats[v].rays.as_dict() for v in variants},
            "lens": _summary(r["lens"]), "pinpoint": _summary(r["pinpoint"]), "camera": _summary(r["camera"]),
            "lens_over_camera": med["lens"] / med["camera"],
            "pinpoint_over_camera": med["pinpoint"] / med["camera"],
            "lens_over_pinpoint": med["lens"] / med["pinpoint"],
        }
        for ds in dss.values():
            ds.close()

    outp = Path(args.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
