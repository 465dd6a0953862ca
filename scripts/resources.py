"""Per-instantiation register/scratch summary of rg_render_kernel.

    python scripts/resources.py [--camera | --lens | --area | --aov | --ao] [extra hipcc flags...]

Compiles the three depth-8 files (rg_render_heavy_d8_host.hip, rg_render_light_d8.hip,
rg_render_heavy_d8.hip) with the library's flags and -Rpass-analysis=kernel-resource-usage and prints VGPRs, spilled VGPRs, scratch bytes per lane, occupancy and static LDS for the
MAXD = 8 instantiations (the ones the bench configurations run; "host": the
host-frame ones, "tpw=-1": the light path's persistent single launches).
--camera: instead, the camera family (MAXD = -1: rg_render_{light,heavy}_camera{,_sparse}.hip) beside
the MAXD = 0 kernels it derives from (rg_render_{light,heavy}_{d0,sparse}.hip), MAXD printed first.
--lens: instead, the lens family (MAXD = -2: rg_render_{light,heavy}_lens.hip) beside the dense camera
kernels it derives from (rg_render_{light,heavy}_camera.hip).
--area: instead, the area family (MAXD = -3: rg_render_{light,heavy}_area.hip) beside the lens family it
derives from (rg_render_{light,heavy}_lens.hip).
--aov: instead, the instantiations of rg_aov_kernel (rg_aov.hip) and the out-of-line sphere_uv they call.
--ao: instead, the instantiations of rg_ao_kernel (rg_ao.hip), SGPR spills (to VGPR lanes, no memory) too."""
import re
import subprocess
import sys
from pathlib import Path

from render_kernel_name import describe, parse

CSRC = Path(__file__).resolve().parent.parent / "raingun_amd" / "csrc"
UNITS = ["rg_render_heavy_d8_host", "rg_render_light_d8", "rg_render_heavy_d8"]
SHOW = (8,)
if "--camera" in sys.argv[1:]:
    sys.argv.remove("--camera")
    UNITS = ["rg_render_light_d0", "rg_render_light_camera", "rg_render_light_sparse", "rg_render_light_camera_sparse",
             "rg_render_heavy_d0", "rg_render_heavy_camera", "rg_render_heavy_sparse", "rg_render_heavy_camera_sparse"]
    SHOW = (0, -1)
if "--lens" in sys.argv[1:]:
    sys.argv.remove("--lens")
    UNITS = ["rg_render_light_camera", "rg_render_light_lens", "rg_render_heavy_camera", "rg_render_heavy_lens"]
    SHOW = (-1, -2)
if "--area" in sys.argv[1:]:
    sys.argv.remove("--area")
    UNITS = ["rg_render_light_lens", "rg_render_light_area", "rg_render_heavy_lens", "rg_render_heavy_area"]
    SHOW = (-2, -3)
AOV = "--aov" in sys.argv[1:]
if AOV:
    sys.argv.remove("--aov")
    UNITS = ["rg_aov"]
AO = "--ao" in sys.argv[1:]
if AO:
    sys.argv.remove("--ao")
    UNITS = ["rg_ao"]
procs = [subprocess.Popen(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                           "-fno-fast-math", "-fPIC", "-c", u + ".hip", "-o", f"/tmp/{u}_res.o",
                           "-Rpass-analysis=kernel-resource-usage", *sys.argv[1:]],
                          cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True) for u in UNITS]
remarks = []
for p, err in [(p, p.communicate()[1]) for p in procs]:
    if p.returncode != 0:
        sys.stderr.write(err[-4000:])
        sys.exit(p.returncode)
    remarks += err.splitlines()
rows, cur = [], None
for line in remarks:
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = {"name": m.group(1)}
        rows.append(cur)
        continue
    m = re.search(r"remark:\s+(VGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
    if m and cur is not None:
        cur[m.group(1)] = int(m.group(2))
for r in rows if AOV else []:
    m = re.match(r"_Z13rg_aov_kernelILb(\d)ELb(\d)ELb(\d)ELb(\d)EE", r["name"])
    if m is None and "sphere_uv" not in r["name"]:
        continue
    what = "sphere_uv (out of line)" if m is None else "rg_aov_kernel<CAMERA %s, F32F %s, BVH %s, SHADE %s>" % m.groups()
    print(f"{what:52s}  VGPRs {r.get('VGPRs')}  spill {r.get('VGPRs Spill')}"
          f"  scratch {r.get('ScratchSize [bytes/lane]')} B/lane  occ {r.get('Occupancy [waves/SIMD]')}  lds {r.get('LDS Size [bytes/block]')}")
for r in rows if AO else []:
    m = re.match(r"_Z12rg_ao_kernelILb(\d)ELb(\d)ELb(\d)EE", r["name"])
    if m is None:
        continue
    what = "rg_ao_kernel<CAMERA %s, F32F %s, BVH %s>" % m.groups()
    print(f"{what:44s}  VGPRs {r.get('VGPRs')}  spill {r.get('VGPRs Spill')}  sgpr spill {r.get('SGPRs Spill')}"
          f"  scratch {r.get('ScratchSize [bytes/lane]')} B/lane  occ {r.get('Occupancy [waves/SIMD]')}  lds {r.get('LDS Size [bytes/block]')}")
for r in [] if AOV or AO else rows:
    k = parse(r["name"])
    if k is None or k["MAXD"] not in SHOW:
        continue
    args = ",".join(str(int(k[n])) for n in ("MAXD", "LSPH", "LCOLD", "WPS", "LBT", "F32F", "BVH", "TASKS"))
    print(f"{describe(k):18s} <{args}>  VGPRs {r.get('VGPRs')}  spill {r.get('VGPRs Spill')}"
          f"  scratch {r.get('ScratchSize [bytes/lane]')} B/lane  occ {r.get('Occupancy [waves/SIMD]')}  lds {r.get('LDS Size [bytes/block]')}")
