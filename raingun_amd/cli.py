"""`raingun` command line, mirroring the reference's src/main.rs + src/render.rs.

    python -m raingun_amd.cli [-w PIXELS] [-h PIXELS] [--4k|--hd] [--draft] [--samples N] [--adaptive T]
                              [--eye X,Y,Z] [--look-at X,Y,Z] [--up X,Y,Z] [--aperture R --focus D]
                              [--light-radius R[,R...]] [--aov LAYERS] [--ao K[,RADIUS[,BIAS]]]
                              [--ambient R,G,B] [--ao-filter R[,NMIN]] [-o FILE] FILE

Flags and their precedence follow construct_app / RenderOptions::from
(main.rs:21-96): --draft forces 800x600 and caps the recursion depth at 4
(main.rs:74-75, 119-123); --hd / --4k set 1920x1080 / 3840x2160 and override
each other (the last one wins); explicit --width/--height override presets
(but not --draft, which clap treats as overriding them, main.rs:47-54).
`--samples N` (1..8, default 1; not in the reference) renders N x N rays per
pixel on the regular sub-pixel grid and box-filters them (rg_render_image_aa);
--draft leaves it alone.  `--adaptive T` (0..256; not in the reference) spends
the N x N rays only on pixels whose 8-neighbourhood contrast in the 1-sample
frame is at least T (rg_render_image_aa_adaptive); with --samples 1 it is
accepted and has no effect.  `--eye X,Y,Z --look-at X,Y,Z [--up X,Y,Z]` (not in
the reference, whose view is from the origin down -z) move the camera
(rg_scene_set_camera): --up defaults to 0,1,0, --eye without --look-at looks
down -z from the eye; a malformed triple or a rejected look-at ends the run
like any other bad flag value.  The scene file has no camera key.
`--aperture R --focus D` (not in the reference) put a thin lens of radius R in
front of the camera, focused on the plane D forward lengths away
(rg_scene_set_lens): depth of field from the N x N rays of --samples, so they
need --samples 2 or more and refuse --adaptive, and go together; they combine
with the camera and the size flags.
`--light-radius R` (not in the reference) gives every spherical light of the
scene the radius R in world units (rg_scene_set_light_radii): soft shadows from
the N x N rays of --samples, so it needs --samples 2 or more and refuses
--adaptive; a comma list gives one radius per light in YAML order (0 for a
directional light).  It combines with the camera and the lens.
`--aov LAYERS` (not in the reference; a comma list of body, depth, normal, uv,
albedo, or `all`) also writes, next to `-o out.png`, `out.<layer>.png` for each
named layer: what lies under each pixel (rg_render_aov), as the pictures of
raingun_amd/aov.py visualize.  It honours the size flags and the camera;
--samples and --adaptive affect only the beauty frame, the layers stay one ray
per pixel.  Without --aov nothing changes, the timing line included.
`--ao K[,RADIUS[,BIAS]]` (not in the reference; K 1..8, RADIUS > 0 or inf, the
default, BIAS >= 0, default 1e-13) also writes `out.ao.png`: the ambient
occlusion of the frame (rg_render_ao), K x K rays over the hemisphere above
each pixel's primary hit, as the grey picture of raingun_amd/ao.py visualize.
It honours the size flags and the camera and is independent of --samples,
--aperture and --light-radius; it runs after the beauty frame and outside its
timing line.  Without --ao nothing changes.
`--ambient R,G,B` (or one number for grey; not in the reference, which has no
ambient light) makes `out.png` the frame of rg_render_image_ambient: the
--samples frame plus this radiance from every open direction, weighted by the
filtered AO pass (raingun_amd/ambient.py).  It needs --ao, refuses --adaptive
and combines with --samples, the camera, the lens and --light-radius.
`--ao-filter R[,NMIN]` (R 0..8, NMIN in [0, 1], default 0.9) is the
edge-stopping filter of the AO pass (rg_ao_filter); it needs --ao.  With
--ambient the default is 2,0.9 and `--ao-filter 0` composes the raw pass; given
explicitly, `out.ao.png` shows the filtered pass.  Without the two flags
nothing changes.  The
render itself runs on the GPU (rg_render_image); the scene is loaded and the
PNG written by the native host layer (libraingun_host.so), and the timing line matches
print_render_message (render.rs:218-244).  `--preview` (piston window) is not
supported: there is no display on an MI355X node.
"""
from __future__ import annotations

import argparse
import sys
import time
from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional

import numpy as np

from . import ambient, ao, aov
from .camera import (Camera, Lens, camera_from_flags, lens_from_flags, light_radii_from_flags, parse_triple,
                     spread_light_radii)


@dataclass
class RenderOptions:          # render.rs:32-46
    width: int = 800
    height: int = 600
    max_recursion_depth: Optional[int] = None
    samples: int = 1          # N x N rays per pixel (--samples; not in the reference)
    adaptive: Optional[int] = None  # contrast threshold of adaptive anti-aliasing (--adaptive)
    camera: Optional[Camera] = None  # --eye / --look-at / --up (not in the reference)
    lens: Optional[Lens] = None      # --aperture / --focus (not in the reference)
    light_radii: Optional[tuple] = None  # --light-radius as given: one number or one per light (not in the reference)
    aov: tuple = ()           # layers of --aov, in aov.LAYERS order (not in the reference)
    ao: Optional[tuple] = None  # --ao as (samples, radius, bias) (not in the reference)
    ambient: Optional[tuple] = None  # --ambient as (r, g, b) (not in the reference)
    ao_filter: Optional[tuple] = None  # --ao-filter as (radius, normal_min), None: not given (not in the reference)


class _LastWins(argparse.Action):
    """clap `overrides_with`: a later flag of the group cancels earlier ones."""

    def __call__(self, parser, ns, values, option_string=None):
        for other in self.const:
            setattr(ns, other, False)
        setattr(ns, self.dest, True)


def construct_app() -> argparse.ArgumentParser:  # main.rs:21-68
    p = argparse.ArgumentParser(prog="raingun", add_help=False,
                                description="Render a raingun YAML scene on an MI355X GPU.")
    p.add_argument("--help", action="help", help="show this help message and exit")
    p.add_argument("-w", "--width", metavar="PIXELS", help="Width of output image.")
    p.add_argument("-h", "--height", metavar="PIXELS", help="Height of output image.")
    p.add_argument("--4k", dest="uhd", action=_LastWins, nargs=0, const=("hd",), default=False,
                   help="Renders in 4K resolution. Explicit width/height overrides.")
    p.add_argument("--hd", dest="hd", action=_LastWins, nargs=0, const=("uhd",), default=False,
                   help="Renders in 1080 (HD) resolution. Explicit width/height overrides.")
    p.add_argument("--draft", action="store_true", help="Renders in 800x600 and lower quality settings.")
    p.add_argument("--preview", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("-o", "--output", metavar="FILENAME",
                   help='Where to save the rendered image. Defaults to input filename with ".png" extension.')
    p.add_argument("--gpu", type=int, default=0, help="HIP device to render on.")
    p.add_argument("--samples", metavar="N",
                   help="Anti-aliasing: N x N rays per pixel on a regular grid, box-filtered (1..8, default 1).")
    p.add_argument("--adaptive", metavar="T",
                   help="Adaptive anti-aliasing: the N x N rays only where the 8-neighbourhood contrast of the "
                        "1-sample frame is at least T (0..256).")
    p.add_argument("--eye", metavar="X,Y,Z", help="Camera position (default 0,0,0).")
    p.add_argument("--look-at", dest="look_at", metavar="X,Y,Z",
                   help="Point the camera looks at (default: straight down -z from the eye).")
    p.add_argument("--up", metavar="X,Y,Z", help="Up hint of --look-at (default 0,1,0).")
    p.add_argument("--aperture", metavar="R", help="Lens radius in world units (with --focus and --samples >= 2).")
    p.add_argument("--focus", metavar="D", help="Distance of the plane in focus, in lengths of the forward vector.")
    p.add_argument("--light-radius", dest="light_radius", metavar="R[,R...]",
                   help="Radius of every spherical light in world units, or one per light (with --samples >= 2).")
    p.add_argument("--aov", metavar="LAYERS",
                   help="Also write FILENAME.<layer>.png for each of a comma list of body, depth, normal, uv, "
                        "albedo (or all).")
    p.add_argument("--ao", metavar="K[,RADIUS[,BIAS]]",
                   help="Also write FILENAME.ao.png: ambient occlusion from K x K rays per pixel (K 1..8) that "
                        "hits within RADIUS occlude (default inf), leaving BIAS above the surface (default 1e-13).")
    p.add_argument("--ambient", metavar="R,G,B",
                   help="Ambient light of this colour (or one number for grey), weighted by the filtered --ao pass, "
                        "added to the frame.")
    p.add_argument("--ao-filter", dest="ao_filter", metavar="R[,NMIN]",
                   help="Edge-stopping filter of the --ao pass: radius 0..8 (0: off) and the least normal cosine "
                        "(default 0.9); with --ambient the default is 2,0.9.")
    p.add_argument("input", metavar="FILE", help="The scene definition file, in YAML format.")
    return p


def options_from(ns: argparse.Namespace) -> RenderOptions:  # main.rs:70-96
    o = RenderOptions()
    if ns.samples is not None:
        o.samples = _parse_u32(ns.samples, "Could not parse samples")
        if not 1 <= o.samples <= 8:
            raise SystemExit("samples must be between 1 and 8")
    if ns.adaptive is not None:
        o.adaptive = _parse_u32(ns.adaptive, "Could not parse adaptive")
        if not 0 <= o.adaptive <= 256:
            raise SystemExit("adaptive must be between 0 and 256")
    o.camera = _parse_camera(ns)
    try:
        o.lens = lens_from_flags(ns.aperture, ns.focus, o.samples, o.adaptive)
    except ValueError as e:
        raise SystemExit(f"Could not build the lens: {e}") from None
    try:
        o.light_radii = light_radii_from_flags(ns.light_radius, o.samples, o.adaptive)
    except ValueError as e:
        raise SystemExit(f"Could not build the area lights: {e}") from None
    if ns.aov is not None:
        try:
            o.aov = aov.parse_layers(ns.aov)
        except ValueError:
            raise SystemExit("Could not parse aov") from None
    if ns.ao is not None:
        try:
            o.ao = ao.parse_spec(ns.ao)
        except ValueError:
            raise SystemExit("Could not parse ao") from None
    if ns.ambient is not None:
        try:
            o.ambient = ambient.parse_spec(ns.ambient)
        except ValueError:
            raise SystemExit("Could not parse ambient") from None
        if o.ao is None:
            raise SystemExit("ambient needs ao")
        if o.adaptive is not None:
            raise SystemExit("ambient cannot be used with adaptive")
    if ns.ao_filter is not None:
        try:
            o.ao_filter = ambient.parse_filter_spec(ns.ao_filter)
        except ValueError:
            raise SystemExit("Could not parse ao-filter") from None
        if o.ao is None:
            raise SystemExit("ao-filter needs ao")
    if ns.draft:
        o.max_recursion_depth = 4
    elif ns.hd:
        o.width, o.height = 1920, 1080
    elif ns.uhd:
        o.width, o.height = 3840, 2160
    if ns.draft:  # --draft overrides width/height (main.rs:47-54)
        return o
    if ns.width is not None:
        o.width = _parse_u32(ns.width, "Could not parse width")
    if ns.height is not None:
        o.height = _parse_u32(ns.height, "Could not parse height")
    return o


def _parse_camera(ns: argparse.Namespace) -> Optional[Camera]:
    triples = {}
    for flag in ("eye", "look_at", "up"):
        text = getattr(ns, flag, None)
        try:
            triples[flag] = None if text is None else parse_triple(text)
        except ValueError:
            raise SystemExit(f"Could not parse {flag.replace('_', '-')}") from None
    try:
        return camera_from_flags(triples["eye"], triples["look_at"], triples["up"])
    except ValueError as e:
        raise SystemExit(f"Could not build the camera: {e}") from None


def _parse_u32(s: str, msg: str) -> int:
    try:
        v = int(s, 10)
    except ValueError:
        raise SystemExit(msg) from None
    if not 0 <= v <= 0xFFFFFFFF:
        raise SystemExit(msg)
    return v


def _join_triples(args: Optional[List[str]]) -> List[str]:
    """`--eye -1,2,3` -> `--eye=-1,2,3`: argparse would read a triple that starts with a minus sign as
    an unknown option."""
    if args is None:
        args = sys.argv[1:]
    out: List[str] = []
    it = iter(args)
    for a in it:
        if a in ("--eye", "--look-at", "--up"):
            v = next(it, None)
            out.append(a if v is None else f"{a}={v}")
        else:
            out.append(a)
    return out


def parse_arguments(args: List[str]) -> RenderOptions:
    return options_from(construct_app().parse_args(_join_triples(args)))


# ---------------------------------------------------------------- PNG (RGBA8)
def encode_png(rgba: np.ndarray) -> bytes:
    """8-bit RGBA PNG through the native encoder (rgh_png_encode, render.rs:58)."""
    from . import _host

    return _host.encode_png(rgba)


def format_duration(ms: int) -> str:  # render.rs:229-244
    one_minute = 1000 * 60
    if 0 <= ms <= 800:
        return f"{ms}ms"
    if 800 < ms <= one_minute:
        return f"{ms / 1000.0:.2f}s"
    minutes = ms // one_minute
    return f"{minutes}m {(ms - minutes * one_minute) / 1000.0:.2f}s"


def main(argv: Optional[List[str]] = None) -> int:  # main.rs:98-132
    ns = construct_app().parse_args(_join_triples(argv))
    opts = options_from(ns)
    if ns.preview:
        print("--preview is not supported on this build (no display); rendering without preview",
              file=sys.stderr)
    input_path = Path(ns.input)
    if ns.output:
        output_path = Path(ns.output)
    else:
        if input_path.suffix == "" and input_path.name in ("", ".", ".."):
            print(f"Could not guess output filename from {input_path}")
            return 2
        output_path = input_path.with_suffix(".png")

    from .scene import load_scene

    if not input_path.exists():
        raise SystemExit("Could not open input file")
    scene = load_scene(input_path)
    if opts.max_recursion_depth is not None and opts.max_recursion_depth < scene.max_recursion_depth:
        scene.max_recursion_depth = opts.max_recursion_depth

    from .scene import DeviceScene

    ds = DeviceScene(scene, device=ns.gpu)
    ds.set_camera(opts.camera)
    ds.set_lens(opts.lens)
    if opts.light_radii is not None:
        from .scene import SphericalLight

        try:
            ds.set_light_radii(spread_light_radii(opts.light_radii, [isinstance(l, SphericalLight) for l in scene.lights]))
        except ValueError as e:
            raise SystemExit(f"Could not build the area lights: {e}") from None
    occlusion = None  # --ambient: the pass it composed (filtered, or raw at --ao-filter 0)
    t0 = time.perf_counter()                     # render.rs:54-56
    if opts.ambient is not None:
        radius, normal_min = opts.ao_filter if opts.ao_filter is not None else ambient.DEFAULT_FILTER
        img, occlusion = ds.render_ambient(opts.width, opts.height, opts.ambient, *opts.ao, samples=opts.samples,
                                           filter_radius=radius, normal_min=normal_min, want_ao=True)
    elif opts.samples > 1 and opts.adaptive is not None:
        img = ds.render_image_aa_adaptive(opts.width, opts.height, opts.samples, opts.adaptive)
    elif opts.samples > 1:
        img = ds.render_image_aa(opts.width, opts.height, opts.samples)
    else:
        img = ds.render_image(opts.width, opts.height)
    t1 = time.perf_counter()
    output_path.write_bytes(encode_png(img))     # render.rs:58
    t2 = time.perf_counter()
    if opts.aov:  # out.png -> out.<layer>.png, one ray per pixel whatever --samples says
        layers = ds.render_aov(opts.width, opts.height, opts.aov)
        for name in opts.aov:
            output_path.with_suffix(f".{name}.png").write_bytes(encode_png(aov.visualize(name, layers[name])))
    if opts.ao is not None:  # out.png -> out.ao.png, whatever --samples, --aperture and --light-radius say
        if opts.ambient is None or opts.ao_filter is None:  # the raw pass; else the pass --ambient composed
            occlusion = ds.render_ao(opts.width, opts.height, *opts.ao)
        if opts.ambient is None and opts.ao_filter is not None and opts.ao_filter[0] > 0:  # the filtered pass
            guides = ds.render_aov(opts.width, opts.height, ("body", "normal"))
            occlusion = ds.filter_ao(occlusion, guides["body"], guides["normal"], *opts.ao_filter)
        output_path.with_suffix(".ao.png").write_bytes(encode_png(ao.visualize(occlusion)))
    ds.close()
    print(f"{input_path}\t→\t{output_path}\t({format_duration(int((t1 - t0) * 1000))} render, "
          f"{format_duration(int((t2 - t1) * 1000))} write)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
