#!/usr/bin/env python3
"""Measure the ambient term on the GPU (separate from bench.py; DESIGN.md 4aa quotes the numbers).

Every time from HIP events on the stream the work runs on, after warm-up, the compared launches alternating in
one process, the median of the timed batches reported with their spread.  test1 (depth 5) and the north-star
scene (1024 spheres, depth 5) at 3840x2160, device-resident, on the scene's own AOV layers and AO pass:

(i)   the filter alone (rg_ao_filter_async) at r = 1, 2, 4, 8, against a floor: a copy kernel that reads the same
      20 B and writes 4 B per pixel (scripts/ambient_floor.hip);
(ii)  the compose alone against its floor (28 B read, 4 B written);
(iii) the whole ambient frame (rg_render_ambient_async, samples 1, filter 2 / 0.9) at k = 2 and k = 4 against its
      three tracing passes measured alone (the sum is reported);
(iv)  AO k = 4 + filter against AO k = 8: the time side of the quality table.

Writes one JSON document (default profiles/ambient/ambient_bench.json) and, with --readme, profiles/ambient/README.md
from it and from the A/B record beside it.  RAINGUN_HIP_LIB selects another build of the library; with
`--ab FILE --key NAME` the run measures the filter alone and stores its medians under NAME in DIR/FILE: the A/B
lines for RG_AOF_PX, RG_AOF_BY, RG_AOF_RECORD and RG_AOF_RUNTIME_R, one process per build, same box, back to back.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import rg_measure as rm
from rg_measure import REPO, summary
PROFILES = REPO / "profiles" / "ambient"
INF = float("inf")
FINITE = {"test1": 8.0, "north_star_1024_spheres": 16.0}
FLOOR_SRC = REPO / "scripts" / "ambient_floor.hip"
FLOOR_LIB = REPO / "scripts" / "bin" / "libambient_floor.so"
RADII = (1, 2, 4, 8)


def build_floor():
    """scripts/bin/libambient_floor.so, built if it is missing or older than its source."""
    if not FLOOR_LIB.exists() or FLOOR_LIB.stat().st_mtime < FLOOR_SRC.stat().st_mtime:
        FLOOR_LIB.parent.mkdir(parents=True, exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-o",
                        str(FLOOR_LIB), str(FLOOR_SRC)], check=True)
    return FLOOR_LIB


def _fmt(r):
    return f"{r['median_ms']:.3f} [{r['min_ms']:.3f} .. {r['max_ms']:.3f}]"


def _readme(result, profiles=PROFILES) -> str:
    lines = ["# profiles/ambient — the ambient term (DESIGN.md §4aa)", "",
             "- `kernel_isa_diff.txt`: every function of the parent commit's device code compiles to the text it had;",
             "  the `rg_ao_filter_kernel` instantiations and `rg_ambient_compose_kernel` are the only new functions.",
             "- `resources.txt`: registers, spills, scratch, occupancy and static LDS of the new kernels.",
             "- `ambient_bench.json`: `python scripts/ambient_bench.py --readme` on one MI355X; the tables below are its summary.",
             "- `ab_filter.json`: `scripts/ambient_bench.py --ab ab_filter.json --key NAME` for builds of rg_ao_filter.hip with",
             "  `-DRG_AOF_BY=.. -DRG_AOF_PX=..` (tile shape, pixels per lane), `-DRG_AOF_RECORD=1` and",
             "  `-DRG_AOF_RUNTIME_R=1`, one process per build, same box, back to back.",
             "- `bench_steps20.json`: `bench.py --gpus 1 --steps 20 --warmup 5` of this build and of the parent commit's",
             "  library, interleaved on one box.", ""]
    if result is None:
        lines += ["None of these figures has been measured yet: `ambient_bench.json` does not exist.", ""]
    else:
        lines += [f"Device: {result['device']}; {result['width']}x{result['height']}; median of {result['batches']} batches of "
                  f"{result['per_batch']} launches (min .. max in brackets), ms.", ""]
        for name, row in result["scenes"].items():
            lines += [f"## {name}", "", "| launch | ms |", "|---|---|"]
            for key, r in row.items():
                if isinstance(r, dict) and "median_ms" in r:
                    lines.append(f"| {key} | {_fmt(r)} |")
            lines.append("")
            for key in ("tracing_sum_k2_ms", "tracing_sum_k4_ms", "ambient_k2_over_tracing", "ambient_k4_over_tracing",
                        "ao_k4_plus_filter_ms", "ao_k4_plus_filter_over_ao_k8", "hit_fraction"):
                if key in row:
                    lines.append(f"- {key}: {row[key]:.4f}")
            lines.append("")
    f = profiles / "ab_filter.json"
    if not f.exists():
        lines += ["A/B of the kernel's open choices: not measured.", ""]
    else:
        lines += ["## A/B of the filter kernel's open choices (`ab_filter.json`; median ms per launch)", "",
                  *rm.ab_table(json.loads(f.read_text()))]
    return "\n".join(lines)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dir", default=str(PROFILES), help="where the records live (default profiles/ambient)")
    ap.add_argument("--out", default=None, help="the JSON document (default DIR/ambient_bench.json)")
    ap.add_argument("--label", default="default build")
    rm.add_timing_args(ap, batches=7, per_batch=5, warmup=1)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--ab", metavar="FILE", help="A/B run: the filter alone, stored under --key in DIR/FILE")
    ap.add_argument("--key", default=None)
    ap.add_argument("--readme", action="store_true", help="also write DIR/README.md")
    ap.add_argument("--readme-only", action="store_true", help="write DIR/README.md from the records and exit")
    args = ap.parse_args(argv)
    profiles = Path(args.dir)
    profiles.mkdir(parents=True, exist_ok=True)
    args.out = args.out or str(profiles / "ambient_bench.json")
    if args.readme_only:
        f = Path(args.out)
        (profiles / "README.md").write_text(_readme(json.loads(f.read_text()) if f.exists() else None, profiles))
        return 0

    import numpy as np
    import torch

    from raingun_amd import _abi, ambient
    from raingun_amd.scene import DeviceScene

    rm.require_gpu("ambient_bench.py")
    lib = _abi.lib()
    floor = None
    if not args.ab:
        floor = C.CDLL(str(build_floor()))
        floor.ambient_floor_filter.argtypes = [C.c_void_p] * 4 + [C.c_uint64, C.c_void_p]
        floor.ambient_floor_compose.argtypes = [C.c_void_p] * 5 + [C.c_uint64, C.c_void_p]
        lib.rg_launch_ambient_compose.restype = C.c_int
        lib.rg_launch_ambient_compose.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.POINTER(C.c_float), C.c_uint64, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]
    stream = torch.cuda.Stream()
    hs = C.c_void_p(stream.cuda_stream)
    W, H = args.width, args.height
    npx = W * H
    batch_ms = rm.event_batch_ms(stream, args.per_batch)

    def measured(fns):
        """The variants alternating -> {name: summary}, the rows of the record."""
        return {k: summary(v) for k, v in rm.alternate(fns, batch_ms, args.warmup, args.batches).items()}

    result = {**rm.header(args, W, H), "scenes": {}}
    scenes = rm.bench_scenes()
    f32 = dict(dtype=torch.float32, device="cuda")
    raw, aof = torch.empty((H, W), **f32), torch.empty((H, W), **f32)
    body = torch.empty((H, W), dtype=torch.int32, device="cuda")
    normal, albedo, rgb = torch.empty((H, W, 3), **f32), torch.empty((H, W, 3), **f32), torch.empty((H, W, 3), **f32)
    rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    layers = _abi.rg_aov(body=body.data_ptr(), normal=normal.data_ptr(), albedo=albedo.data_ptr())
    color = (C.c_float * 3)(0.3, 0.25, 0.45)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    with torch.cuda.stream(stream):
        for name, scene in scenes.items():
            ds = DeviceScene(scene)
            share = torch.from_numpy(np.ascontiguousarray(ambient.shares(scene))).cuda()

            la = rm.Launches(ds, W, H, stream)

            def launch_ao(k, radius=INF, stats=None):
                la.ao(_abi.rg_ao(k, 0, radius, 1e-13), raw, stats)

            def launch_aov():
                la.aov(layers)

            def launch_beauty():
                la.aa(1, rgba, rgb)

            def launch_filter(r, nmin=0.9):
                f = _abi.rg_ao_filter_desc(r, nmin)
                _abi.check(lib.rg_ao_filter_async(0, p(raw), p(body), p(normal), W, H, C.byref(f), p(aof), hs))

            def launch_compose():
                assert lib.rg_launch_ambient_compose(p(rgb), p(albedo), p(body), p(aof), p(share), share.numel(), color, npx,
                                                     p(rgba), None, hs) == 0

            def launch_ambient(k):
                m = _abi.rg_ambient(color, 1, _abi.rg_ao(k, 0, INF, 1e-13), 2, 0.9)
                _abi.check(lib.rg_render_ambient_async(ds.handle, W, H, C.byref(m), p(rgba), None, None, hs, None))

            # the layers every image-space launch below reads: this scene's own
            st = _abi.rg_stats()
            launch_aov()
            launch_beauty()
            launch_ao(4, INF, st)
            row = {"hit_fraction": int(st.rays.shadow) / 16 / npx}
            fns = {f"filter_r{r}": (lambda r=r: launch_filter(r)) for r in RADII}
            if args.ab:
                row.update(measured(fns))
            else:
                fns["filter_floor"] = lambda: floor.ambient_floor_filter(p(raw), p(body), p(normal), p(aof), npx, hs)
                row.update(measured(fns))
                launch_filter(2)
                row.update(measured({
                    "compose": launch_compose,
                    "compose_floor": lambda: floor.ambient_floor_compose(p(rgb), p(albedo), p(body), p(aof), p(rgba), npx, hs)}))
                row.update(measured({
                    "ambient_frame_k2": lambda: launch_ambient(2), "ambient_frame_k4": lambda: launch_ambient(4),
                    "beauty_samples1_rgb": launch_beauty, "aov_body_normal_albedo": launch_aov,
                    "ao_k2_inf": lambda: launch_ao(2), "ao_k4_inf": lambda: launch_ao(4), "ao_k8_inf": lambda: launch_ao(8),
                    "ao_k4_then_filter_r2": lambda: (launch_ao(4), launch_filter(2))}))
                tracing = row["beauty_samples1_rgb"]["median_ms"] + row["aov_body_normal_albedo"]["median_ms"]
                for k in (2, 4):
                    row[f"tracing_sum_k{k}_ms"] = tracing + row[f"ao_k{k}_inf"]["median_ms"]
                    row[f"ambient_k{k}_over_tracing"] = row[f"ambient_frame_k{k}"]["median_ms"] / row[f"tracing_sum_k{k}_ms"]
                row["ao_k4_plus_filter_ms"] = row["ao_k4_then_filter_r2"]["median_ms"]
                row["ao_k4_plus_filter_over_ao_k8"] = row["ao_k4_then_filter_r2"]["median_ms"] / row["ao_k8_inf"]["median_ms"]
            assert ds.stream_status(stream.cuda_stream) == (0, -1)
            result["scenes"][name] = row
            ds.release_stream(stream.cuda_stream)
            ds.close()

    if args.ab:
        f = profiles / args.ab
        ab = json.loads(f.read_text()) if f.exists() else {}
        key = args.key or args.label
        ab[key] = {f"{name.split('_')[0]} {k}": v for name, row in result["scenes"].items() for k, v in row.items()
                   if isinstance(v, dict)}
        f.write_text(json.dumps(ab, indent=1) + "\n")
        print(json.dumps({key: {k: round(v["median_ms"], 4) for k, v in ab[key].items()}}))
        return 0
    rm.write_record(result, args.out)
    if args.readme:
        (profiles / "README.md").write_text(_readme(result, profiles))
    return 0


if __name__ == "__main__":
    sys.exit(main())
