#!/usr/bin/env python3
"""Measure the ambient occlusion pass on the GPU (separate from bench.py; DESIGN.md 4z quotes the numbers).

Every time from HIP events on the stream the work runs on, after warm-up, the compared launches alternating in
one process, the median of the timed batches reported with their spread.  test1 (depth 5) and the north-star
scene (1024 spheres, depth 5) at 3840x2160, device-resident single launches under the fixed view:

(i)   rg_render_ao_async with k = 2 and k = 4, radius +inf and one finite radius (test1: 8, north star: 16):
      ms per frame and AO rays per second (the launch's own shadow-class count over its time);
(ii)  rg_render_aov_async, body + depth: the floor, the primary rays alone;
(iii) the same scene's rg_render_tiles_async beauty frame with its rays per second: the project's own any-hit
      rate (its shadow rays are the coherent kind, towards a handful of lights).

Writes one JSON document (default profiles/ao/ao_bench.json) and, with --readme, profiles/ao/README.md from it
and from the A/B records beside it.  RAINGUN_HIP_LIB selects another build of the library; with
`--ab FILE --key NAME` the run measures AO alone (k = 4, +inf and the finite radius) and stores its medians under NAME in
DIR/FILE: the A/B lines for RG_AO_TILE_WLOG, RG_AO_BLOCKS_PER_CU and RG_AO_LANE_WALK, one process per
build, same box, back to back.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import rg_measure as rm
from rg_measure import REPO, summary
PROFILES = REPO / "profiles" / "ao"
INF = float("inf")
FINITE = {"test1": 8.0, "north_star_1024_spheres": 16.0}


def _readme(result, PROFILES=PROFILES) -> str:
    lines = ["# profiles/ao — the ambient occlusion pass (DESIGN.md §4z)", "",
             "- `kernel_isa_diff.txt`: every function of the parent commit's device code compiles to the text it had;",
             "  the six `rg_ao_kernel` instantiations are the only new functions.",
             "- `resources.txt`: `python scripts/resources.py --ao`, registers, spills, scratch, occupancy and static LDS",
             "  of the six instantiations.",
             "- `ao_bench.json`: `python scripts/ao_bench.py --readme` on one MI355X; the table below is its summary.",
             "- `ab_tile_shape.json`, `ab_grid.json`, `ab_walk.json`: `scripts/ao_bench.py --ab FILE --key NAME` for builds",
             "  with `-DRG_AO_TILE_WLOG=3..6`, `-DRG_AO_BLOCKS_PER_CU=..` and `-DRG_AO_LANE_WALK=0/1` (AO alone, k = 4,",
             "  radius +inf and the finite one), one process per build, same box, back to back.",
             "- `bench_steps20.json`: `bench.py --gpus 1 --steps 20 --warmup 5` of this build.", ""]
    if result is None:
        lines += ["None of these figures has been measured yet: `ao_bench.json` does not exist.", ""]
        return "\n".join(lines)
    lines += [f"Device: {result['device']}; {result['width']}x{result['height']}; median of {result['batches']} batches of "
              f"{result['per_batch']} launches (min .. max in brackets).", "",
              "| scene | launch | ms per frame | rays of the class | G rays/s |", "|---|---|---|---|---|"]
    for name, rows in result["scenes"].items():
        for key, r in rows.items():
            if not isinstance(r, dict) or "median_ms" not in r:
                continue
            rays = r.get("rays")
            rate = f"{r['grays_per_s']:.2f}" if "grays_per_s" in r else ""
            lines.append(f"| {name} | {key} | {r['median_ms']:.3f} [{r['min_ms']:.3f} .. {r['max_ms']:.3f}] | "
                         f"{rays if rays is not None else ''} | {rate} |")
    lines.append("")
    for fname, what in (("ab_tile_shape.json", "tile shape"), ("ab_grid.json", "blocks per CU"), ("ab_walk.json", "walk kind")):
        f = PROFILES / fname
        if not f.exists():
            lines += [f"A/B {what}: not measured.", ""]
            continue
        ab = json.loads(f.read_text())
        lines += [f"A/B {what} (`{fname}`; AO k = 4, median ms per frame):", "", *rm.ab_table(ab)]
    return "\n".join(lines)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dir", default=str(PROFILES), help="where the records live (default profiles/ao)")
    ap.add_argument("--out", default=None, help="the JSON document (default DIR/ao_bench.json)")
    ap.add_argument("--label", default="default build")
    rm.add_timing_args(ap, batches=5, per_batch=3, warmup=1)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--ab", metavar="FILE", help="A/B run: AO alone (k = 4), stored under --key in profiles/ao/FILE")
    ap.add_argument("--key", default=None)
    ap.add_argument("--readme", action="store_true", help="also write profiles/ao/README.md")
    ap.add_argument("--readme-only", action="store_true", help="write profiles/ao/README.md from the records and exit")
    args = ap.parse_args(argv)
    profiles = Path(args.dir)
    profiles.mkdir(parents=True, exist_ok=True)
    args.out = args.out or str(profiles / "ao_bench.json")
    if args.readme_only:
        f = Path(args.out)
        (profiles / "README.md").write_text(_readme(json.loads(f.read_text()) if f.exists() else None, profiles))
        return 0

    import torch

    from raingun_amd import _abi
    from raingun_amd.scene import DeviceScene

    rm.require_gpu("ao_bench.py")
    stream = torch.cuda.Stream()
    W, H = args.width, args.height
    batch_ms = rm.event_batch_ms(stream, args.per_batch)
    result = {**rm.header(args, W, H), "scenes": {}}
    scenes = rm.bench_scenes()
    out = torch.empty((H, W), dtype=torch.float32, device="cuda")
    body = torch.empty((H, W), dtype=torch.int32, device="cuda")
    depth = torch.empty((H, W), dtype=torch.float64, device="cuda")
    rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    v_bd = _abi.rg_aov(body=body.data_ptr(), depth=depth.data_ptr())

    with torch.cuda.stream(stream):
        for name, scene in scenes.items():
            ds = DeviceScene(scene)
            la = rm.Launches(ds, W, H, stream)
            passes = {"ao_k4_inf": _abi.rg_ao(4, 0, INF, 1e-13), "ao_k4_finite": _abi.rg_ao(4, 0, FINITE[name], 1e-13)}
            if not args.ab:
                passes.update({"ao_k2_inf": _abi.rg_ao(2, 0, INF, 1e-13), "ao_k2_finite": _abi.rg_ao(2, 0, FINITE[name], 1e-13)})
            rays = {}
            for key, v in passes.items():  # one counted launch each: the rays of the class
                st = _abi.rg_stats()
                la.ao(v, out, st)
                assert st.rays.primary == W * H and st.rays.secondary == 0 and st.rays.shadow % (v.samples ** 2) == 0
                rays[key] = int(st.rays.shadow)
            fns = {key: (lambda v=v: la.ao(v, out)) for key, v in passes.items()}
            if not args.ab:
                st = _abi.rg_stats()
                la.frame(rgba, stats=st)
                rays["frame_depth5"] = int(st.rays.primary + st.rays.shadow + st.rays.secondary)
                frame_shadow = int(st.rays.shadow)
                rays["aov_body_depth"] = W * H
                fns["aov_body_depth"] = lambda: la.aov(v_bd)
                fns["frame_depth5"] = lambda: la.frame(rgba)
            r = rm.alternate(fns, batch_ms, args.warmup, args.batches)
            assert ds.stream_status(stream.cuda_stream) == (0, -1)
            row = {}
            for key, ms in r.items():
                row[key] = summary(ms)
                row[key]["rays"] = rays[key]
                row[key]["grays_per_s"] = rays[key] / statistics.median(ms) / 1e6
            if not args.ab:
                row["frame_depth5"]["shadow_rays"] = frame_shadow
                row["hit_fraction"] = rays["ao_k4_inf"] / 16 / (W * H)
                floor = row["aov_body_depth"]["median_ms"]
                for key in passes:  # AO rays per second with the primary pass's time taken off
                    row[key]["grays_per_s_above_floor"] = rays[key] / max(row[key]["median_ms"] - floor, 1e-9) / 1e6
            result["scenes"][name] = row
            ds.close()

    if args.ab:
        f = profiles / args.ab
        ab = json.loads(f.read_text()) if f.exists() else {}
        ab[args.key or args.label] = {f"{name} {key[6:]}": row[key] for name, row in result["scenes"].items()
                                      for key in ("ao_k4_inf", "ao_k4_finite")}
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(json.dumps(ab, indent=1) + "\n")
        print(json.dumps({args.key or args.label: ab[args.key or args.label]}))
        return 0
    rm.write_record(result, args.out)
    if args.readme:
        (profiles / "README.md").write_text(_readme(result, profiles))
    return 0


if __name__ == "__main__":
    sys.exit(main())
