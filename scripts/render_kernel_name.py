"""The mangled name of an rg_render_kernel instantiation <-> its named template parameters
(raingun_amd/csrc/rg_render_cfg.h says what they mean).  For the scripts that pick kernels out of
compiler remarks, assembly and profiles: scripts/resources.py, scripts/isa_budget.py.

    parse(name)    -> {"MAXD": 8, "LSPH": True, ...}, or None if name is no rg_render_kernel
    mangle(**p)    -> the name
    describe(p)    -> "light", "heavy host", "light tpw=-1 plain", "heavy camera sparse", "light lens", "heavy area", ...

MAXD: array frames per lane; 0: frames in the global buffer; MAXD_CAMERA (-1, mangled Lin1E): the same
with the primary rays of a movable camera (the camera family); MAXD_LENS (-2, mangled Lin2E): those
through a thin lens (the lens family); MAXD_AREA (-3, mangled Lin3E): the lens family's kernels with area
lights (the area family).
"""
import re

# (name, is_int) in the template's order
PARAMS = [("MAXD", True), ("LSPH", False), ("LCOLD", False), ("WPS", True), ("LBT", True), ("F32F", False),
          ("BVH", False), ("TASKS", False), ("TPW", True), ("HF", False), ("SPARSE", False), ("PLAIN", False)]
MAXD_CAMERA = -1
MAXD_LENS = -2
MAXD_AREA = -3
_ARG = {True: r"Li(n?\d+)E", False: r"Lb([01])E"}
_NAME = re.compile("^_Z16rg_render_kernelI" + "".join(_ARG[i] for _, i in PARAMS) + "Ev12RgKernelArgs$")


def parse(name):
    m = _NAME.match(name)
    if not m:
        return None
    return {n: int(v.replace("n", "-")) if is_int else v == "1" for (n, is_int), v in zip(PARAMS, m.groups())}


def mangle(**p):
    assert sorted(p) == sorted(n for n, _ in PARAMS), sorted(p)
    args = "".join(f"Li{str(int(p[n])).replace('-', 'n')}E" if is_int else f"Lb{int(bool(p[n]))}E" for n, is_int in PARAMS)
    return f"_Z16rg_render_kernelI{args}Ev12RgKernelArgs"


def describe(p):
    """Kind of kernel, as scripts/resources.py prints it (LBT 1: the heavy path; TPW < 0: persistent waves)."""
    kind = "heavy" if p["LBT"] == 1 else "light"
    if p["TPW"] != 0:
        kind += f" tpw={p['TPW']}"
    if p["HF"]:
        kind += " host"
    if p["MAXD"] == MAXD_CAMERA:
        kind += " camera"
    if p["MAXD"] == MAXD_LENS:
        kind += " lens"
    if p["MAXD"] == MAXD_AREA:
        kind += " area"
    if p["SPARSE"]:
        kind += " sparse"
    if p["PLAIN"]:
        kind += " plain"
    return kind


# the kernel of the headline benchmark (test1 at 4K, three lights): the PLAIN light kernel, 8 array frames
HEADLINE = mangle(MAXD=8, LSPH=True, LCOLD=True, WPS=4, LBT=3, F32F=False, BVH=False, TASKS=False, TPW=0, HF=False,
                  SPARSE=False, PLAIN=True)
