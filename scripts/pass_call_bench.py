#!/usr/bin/env python3
"""Host time per call of the pixel passes' entry points (separate from bench.py; profiles/passes quotes the numbers).

The kernels of rg_render_aov_async, rg_render_ao_async and rg_render_ambient_async are what aov_bench.py,
ao_bench.py and ambient_bench.py time with HIP events.  This script times the CALL, on the host clock, at a
frame small enough (test1, depth 5, 320x180) that the host path is what is measured:

- without `stats` the call only enqueues: wall time of a batch of calls over their number, the stream
  synchronised (untimed) between batches;
- with `stats` the call waits for its launch and reads the counters back: wall time per call, the same way.

One JSON document on stdout and, with --out, in a file: per entry and mode the median, minimum and maximum of the
batches, in microseconds per call.  RAINGUN_HIP_LIB selects another build of the library; an A/B of two builds
runs this script once per build, alternating, in one job on one device, and compares the medians with the
run-to-run spread of one build's own repeats.
"""
from __future__ import annotations

import argparse
import ctypes as C
import statistics
import sys
import time

import rg_measure as rm


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the JSON document there")
    ap.add_argument("--label", default="default build")
    rm.add_timing_args(ap, batches=50, per_batch=10, warmup=2)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=180)
    args = ap.parse_args(argv)

    import torch

    from raingun_amd import _abi
    from raingun_amd.scene import DeviceScene

    rm.require_gpu("pass_call_bench.py")
    lib = _abi.lib()
    stream = torch.cuda.Stream()
    hs = C.c_void_p(stream.cuda_stream)
    W, H = args.width, args.height
    whole = _abi.rg_tiling(H, 1, 0)
    ds = DeviceScene(rm.bench_scenes()["test1"])

    def p(t):
        return C.c_void_p(t.data_ptr())

    body = torch.empty((H, W), dtype=torch.int32, device="cuda")
    depth = torch.empty((H, W), dtype=torch.float64, device="cuda")
    ao = torch.empty((H, W), dtype=torch.float32, device="cuda")
    rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    v_aov = _abi.rg_aov(body=body.data_ptr(), depth=depth.data_ptr())
    v_ao = _abi.rg_ao(2, 0, float("inf"), 1e-13)
    color = (C.c_float * 3)(0.2, 0.2, 0.2)
    v_amb = _abi.rg_ambient(color, 1, v_ao, 2, 0.9)
    st = _abi.rg_stats()

    entries = {
        "aov_async": lambda s: lib.rg_render_aov_async(ds.handle, W, H, C.byref(whole), C.byref(v_aov), hs, s),
        "ao_async": lambda s: lib.rg_render_ao_async(ds.handle, W, H, C.byref(whole), C.byref(v_ao), p(ao), hs, s),
        "ambient_async": lambda s: lib.rg_render_ambient_async(ds.handle, W, H, C.byref(v_amb), p(rgba), None, None, hs, s),
    }

    def batch_us(fn, s):
        t0 = time.perf_counter()
        for _ in range(args.per_batch):
            fn(s)
        t1 = time.perf_counter()
        stream.synchronize()
        return (t1 - t0) / args.per_batch * 1e6

    result = {**rm.header(args, W, H), "us_per_call": {}}
    for name, fn in entries.items():
        for mode, s in (("no_stats", None), ("stats", C.byref(st))):
            _abi.check(fn(s))
            for _ in range(args.warmup):
                batch_us(fn, s)
            us = [batch_us(fn, s) for _ in range(args.batches)]
            result["us_per_call"][f"{name} {mode}"] = {"median": statistics.median(us), "min": min(us), "max": max(us)}
    assert ds.stream_status(stream.cuda_stream) == (0, -1)
    ds.close()
    rm.write_record(result, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
