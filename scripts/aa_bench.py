#!/usr/bin/env python3
"""Measure supersampled anti-aliasing on the GPU (separate from bench.py).

Three things, every time from HIP events on the stream the work runs on (or, for
the blocking host entry, a host clock around the call, which ends in a
synchronise), after warm-up, the compared pair alternating in one process:

1. the resolve kernel alone (rg_launch_resolve) for a 3840x2160 output at
   samples = 2 and 4, with and without the f32 output, its bytes moved
   (12 k^2 W H read + 4 W H (+ 12 W H) written), beside a hipMemcpyDtoDAsync of
   the same total traffic (copy size = half of read plus written);
2. rg_render_aa_async of test1 (depth 5) at 1920x1080, samples = 2, beside
   rg_render_tiles_async of the same scene at 3840x2160: the same rays, the
   difference is the scratch writes plus the resolve;
3. rg_render_image_aa of the same case into page-locked host memory.

Writes one JSON document (default profiles/aa/aa_bench.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
import functools
import statistics
import sys
import time

import rg_measure as rm
from rg_measure import REPO, summary


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(REPO / "profiles" / "aa" / "aa_bench.json"))
    rm.add_timing_args(ap, batches=7, per_batch=10, warmup=3)
    ap.add_argument("--band-rows", type=int, default=0, help="rg_debug_set_aa_band_rows (0: automatic)")
    ap.add_argument("--skip-resolve", action="store_true", help="only the render measurements (band-size sweeps)")
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    from raingun_amd import _abi
    from raingun_amd.scene import DeviceScene

    rm.require_gpu("aa_bench.py")
    lib = _abi.lib()
    lib.rg_launch_resolve.restype = C.c_int
    lib.rg_launch_resolve.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hipMemcpyDtoDAsync.restype = C.c_int  # the HIP runtime the library is linked to (one per process)
    lib.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    stream = torch.cuda.Stream()
    hs = C.c_void_p(stream.cuda_stream)

    alternate = functools.partial(rm.alternate, batch_ms=rm.event_batch_ms(stream, args.per_batch),
                                  warmup=args.warmup, batches=args.batches)
    result = {**rm.header(args), "resolve": [], "render": {}}

    # ---------------------------------------------------------------- 1. the resolve kernel alone
    W, H = 3840, 2160
    for k in () if args.skip_resolve else (2, 4):
        samples = torch.rand((k * H, k * W, 3), dtype=torch.float32, device="cuda") * 1.5 - 0.25
        rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
        rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        for want_rgb in (False, True):
            read_b = 12 * k * k * W * H
            write_b = 4 * W * H + (12 * W * H if want_rgb else 0)
            copy_b = (read_b + write_b) // 2
            src = torch.empty(copy_b, dtype=torch.uint8, device="cuda")
            dst = torch.empty(copy_b, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()

            def resolve():
                e = lib.rg_launch_resolve(samples.data_ptr(), W, H, k, rgba.data_ptr(),
                                          rgb.data_ptr() if want_rgb else None, hs)
                assert e == 0, e

            def copy():
                e = lib.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), copy_b, hs)
                assert e == 0, e

            r = alternate({"resolve": resolve, "copy": copy})
            res_ms, copy_ms = statistics.median(r["resolve"]), statistics.median(r["copy"])
            result["resolve"].append({
                "width": W, "height": H, "samples": k, "f32_output": want_rgb,
                "bytes_read": read_b, "bytes_written": write_b,
                "resolve": summary(r["resolve"]), "copy_same_traffic": summary(r["copy"]),
                "resolve_tb_per_s": (read_b + write_b) / (res_ms * 1e-3) / 1e12,
                "copy_tb_per_s": 2 * copy_b / (copy_ms * 1e-3) / 1e12,
                "resolve_over_copy": res_ms / copy_ms,
            })
            del src, dst
        del samples, rgba, rgb
        torch.cuda.empty_cache()

    # ---------------------------------------------------------------- 2. / 3. the render
    ds = DeviceScene(rm.bench_scenes()["test1"])
    ds.set_aa_band_rows(args.band_rows)
    w, h, k = 1920, 1080, 2
    aa_rgba = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    big_rgba = torch.empty((k * h, k * w, 4), dtype=torch.uint8, device="cuda")
    out_size, sample_size = rm.Launches(ds, w, h, stream), rm.Launches(ds, k * w, k * h, stream)
    r = alternate({"aa": lambda: out_size.aa(k, aa_rgba), "plain": lambda: sample_size.frame(big_rgba)})
    aa_ms, plain_ms = statistics.median(r["aa"]), statistics.median(r["plain"])
    st = _abi.rg_stats()
    out_size.aa(k, aa_rgba, stats=st)
    result["render"] = {
        "scene": "test1", "max_depth": 5, "width": w, "height": h, "samples": k, "band_rows": args.band_rows,
        "rays": st.rays.total(),
        "rg_render_aa_async": summary(r["aa"]),
        "rg_render_tiles_async_at_sample_size": summary(r["plain"]),
        "scratch_and_resolve_ms": aa_ms - plain_ms,
        "stats_kernel_ms_one_frame": st.kernel_ms,
    }

    # page-locked host destination: blocking calls, a host clock around each
    pinned = torch.empty((h, w, 4), dtype=torch.uint8).pin_memory()
    out = pinned.numpy()
    host_ms = []
    for i in range(args.warmup * args.per_batch + args.batches * args.per_batch):
        t0 = time.perf_counter()
        ds.render_image_aa(w, h, k, out=out)
        t1 = time.perf_counter()
        if i >= args.warmup * args.per_batch:
            host_ms.append((t1 - t0) * 1e3)
    assert np.array_equal(out, aa_rgba.cpu().numpy()), "host and device-resident frames differ"
    result["render"]["rg_render_image_aa_pinned"] = {"median_ms": statistics.median(host_ms), "min_ms": min(host_ms),
                                                     "max_ms": max(host_ms), "calls": len(host_ms)}
    ds.close()

    rm.write_record(result, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
