#!/usr/bin/env python3
"""Measure the movable camera on the GPU (separate from bench.py; DESIGN.md 4s quotes the numbers).

Every time from HIP events on the stream the work runs on, after warm-up, the compared pair
alternating in one process, the median of the timed batches reported:

1. the price of general primary rays: test1 (depth 5) and the north-star scene (1024 spheres,
   depth 5) at 3840x2160, device-resident (rg_render_tiles_async), with the IDENTITY camera set --
   the camera kernels, whose primary rays go through the general closest-hit query, without PLAIN
   and without the camera buffer -- against the same frames without a camera (the kernels the
   library ran before it had cameras, which it still contains).  The two frames are compared
   byte for byte first.
2. a 64-frame orbit around the north-star scene, 8 frames in flight on 8 streams through
   rg_render_tiles_pipelined, one rg_scene_set_camera per frame: ms per frame, and the host's
   enqueue cost per frame (a host clock around set_camera + the launch call).  Nothing to compare
   it with; the same loop without a camera is timed beside it for scale.

Writes one JSON document (default profiles/camera/camera_bench.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import statistics
import sys
import time

import rg_measure as rm
from rg_measure import REPO, summary


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(REPO / "profiles" / "camera" / "camera_bench.json"))
    rm.add_timing_args(ap, batches=7, per_batch=10, warmup=3)
    ap.add_argument("--orbit-frames", type=int, default=64)
    ap.add_argument("--in-flight", type=int, default=8)
    args = ap.parse_args(argv)

    import torch

    from raingun_amd import _abi
    from raingun_amd.camera import Camera
    from raingun_amd.scene import DeviceScene

    rm.require_gpu("camera_bench.py")
    lib = _abi.lib()
    stream = torch.cuda.Stream()
    W, H = 3840, 2160
    whole = _abi.rg_tiling(H, 1, 0)

    batch_ms = rm.event_batch_ms(stream, args.per_batch)
    result = {**rm.header(args, W, H), "identity_camera": {}, "orbit": {}}
    scenes = rm.bench_scenes()
    buf = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    buf2 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")

    # ---------------------------------------------------------------- 1. identity camera against no camera
    for name, scene in scenes.items():
        fixed, moved = DeviceScene(scene), DeviceScene(scene)
        moved.set_camera(Camera.identity())
        lf, lm = rm.Launches(fixed, W, H, stream), rm.Launches(moved, W, H, stream)
        st0, st1 = _abi.rg_stats(), _abi.rg_stats()
        lf.frame(buf, stats=st0)
        plain = fixed.last_plain()
        lm.frame(buf2, stats=st1)
        assert torch.equal(buf, buf2), "the identity camera's frame differs"
        assert st0.rays.as_dict() == st1.rays.as_dict()
        r = rm.alternate({"fixed": lambda: lf.frame(buf), "camera": lambda: lm.frame(buf2)},
                         batch_ms, args.warmup, args.batches)
        f_ms, c_ms = statistics.median(r["fixed"]), statistics.median(r["camera"])
        result["identity_camera"][name] = {
            "max_depth": 5, "rays": st0.rays.total(), "fixed_view_ran_plain": bool(plain),
            "fixed_view": summary(r["fixed"]), "identity_camera": summary(r["camera"]),
            "camera_over_fixed": c_ms / f_ms, "camera_minus_fixed_ms": c_ms - f_ms,
        }
        fixed.close()
        moved.close()

    # ---------------------------------------------------------------- 2. an orbit with frames in flight
    ds = DeviceScene(scenes["north_star_1024_spheres"])
    n, depth = args.orbit_frames, args.in_flight
    streams = [torch.cuda.Stream() for _ in range(depth)]
    bufs = [torch.empty((H, W, 4), dtype=torch.uint8, device="cuda") for _ in range(depth)]
    centre, radius, height = (0.0, 5.0, -49.0), 75.0, 18.0
    cams = []
    for k in range(n):
        a = 2.0 * math.pi * k / n
        eye = (centre[0] + radius * math.sin(a), centre[1] + height, centre[2] + radius * math.cos(a))
        cams.append(Camera.look_at(eye, centre))

    def orbit(with_camera):
        """-> (ms per frame by HIP events over the whole loop, host enqueue us per frame)"""
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(streams[0])
        for s in streams[1:]:
            s.wait_event(e0)
        host = 0.0
        for k in range(n):
            s, b = streams[k % depth], bufs[k % depth]
            t0 = time.perf_counter()
            if with_camera:
                ds.set_camera(cams[k])
            _abi.check(lib.rg_render_tiles_pipelined(ds.handle, W, H, C.byref(whole), C.c_void_p(b.data_ptr()), None,
                                                     C.c_void_p(s.cuda_stream)))
            host += time.perf_counter() - t0
        for s in streams[1:]:
            ev = torch.cuda.Event()
            ev.record(s)
            streams[0].wait_event(ev)
        e1.record(streams[0])
        e1.synchronize()
        return e0.elapsed_time(e1) / n, host / n * 1e6

    res = {"camera": ([], []), "fixed": ([], [])}
    ds.set_camera(None)
    for _ in range(args.warmup):
        orbit(True)
        ds.set_camera(None)
        orbit(False)
    for _ in range(args.batches):
        for key, with_camera in (("camera", True), ("fixed", False)):
            ds.set_camera(None)
            ms, us = orbit(with_camera)
            res[key][0].append(ms)
            res[key][1].append(us)
    for s in streams:
        st, px = ds.stream_status(s.cuda_stream)
        assert st == 0, (st, px)
    result["orbit"] = {
        "scene": "north_star_1024_spheres", "frames": n, "in_flight": depth, "radius": radius,
        "orbit_ms_per_frame": summary(res["camera"][0]),
        "orbit_host_enqueue_us_per_frame": statistics.median(res["camera"][1]),
        "fixed_view_same_loop_ms_per_frame": summary(res["fixed"][0]),
        "fixed_view_host_enqueue_us_per_frame": statistics.median(res["fixed"][1]),
    }
    for s in streams:
        ds.release_stream(s.cuda_stream)
    ds.close()

    rm.write_record(result, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
