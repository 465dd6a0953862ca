"""Host-side mirror of raingun-lib's public API (scene.rs, bodies.rs, lights.rs,
material.rs) above the C ABI of libraingun_hip.so.

* :func:`load_scene` runs the native C++ loader (include/raingun_host.h), which
  reproduces the serde schema of `Scene` (scene.rs:11-31) as serde_yaml 0.6
  over yaml-rust 0.3.5 reads it: camelCase top-level keys with
  `deny_unknown_fields`; externally tagged enums (`Sphere:`/`Plane:`/`Disk:`/
  `AABB:`, `Directional:`/`Spherical:`, `Color:`/`Texture:`, `Diffuse` /
  `{Diffuse: null}` / `{Reflecting: {...}}` / `{Refractive: {...}}`); Point3 and
  Vector3 as `[x, y, z]` or `{x:, y:, z:}` (cgmath "eders"); f32 fields rounded
  to f32; textures decoded eagerly at load time relative to the working
  directory (material.rs:34-47) by the native decoder (libraingun_host.so),
  which rounds like the reference's jpeg-decoder 0.1.11.  This module only
  converts the loaded rg_scene_desc into the dataclasses below.
* :class:`Scene` keeps the reference's `render_image(width, height)` /
  `streaming_render(...)` / `trace(ray)` entry points (scene.rs:34-51); every
  one of them runs on the GPU through the C ABI.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from pathlib import Path
from typing import Callable, List, Optional, Sequence, Union

import numpy as np

from . import _abi, aov
from .camera import Camera, Lens
from .color import Color



class SceneError(ValueError):
    """The YAML does not deserialise into a Scene (serde_yaml's Err)."""


# ---------------------------------------------------------------- data model
@dataclass
class Texture:                 # material.rs:26-32
    path: str
    image: np.ndarray          # (h, w, 4) uint8 RGBA
    x_offset: float
    y_offset: float


@dataclass
class Material:                # material.rs:7-12
    coloration: Union[Color, Texture]
    albedo: float
    surface: str = "Diffuse"   # Diffuse | Reflecting | Refractive
    reflectivity: float = 0.0
    index: float = 0.0
    transparency: float = 0.0


@dataclass
class Sphere:                  # bodies.rs:13-18
    center: tuple
    radius: float
    material: Material


@dataclass
class Plane:                   # bodies.rs:20-25
    origin: tuple
    normal: tuple
    material: Material


@dataclass
class Disk:                    # bodies.rs:27-33
    origin: tuple
    normal: tuple
    radius: float
    material: Material


@dataclass
class AABB:                    # bodies.rs:35-39
    bounds: tuple              # ((x0,y0,z0), (x1,y1,z1))
    material: Material


@dataclass
class DirectionalLight:        # lights.rs:8-13
    direction: tuple
    color: Color
    intensity: float


@dataclass
class SphericalLight:          # lights.rs:15-20
    position: tuple
    color: Color
    intensity: float


Body = Union[Sphere, Plane, Disk, AABB]
Light = Union[DirectionalLight, SphericalLight]


# ---------------------------------------------------------------- loading
def load_scene(source: Union[str, os.PathLike], texture_root: Optional[Union[str, os.PathLike]] = None) -> "Scene":
    """serde_yaml::from_reader::<Scene> (main.rs:116-118) through the native
    loader (rgh_scene_load_*, raingun_amd/host/scene_loader.cpp).  `source` is
    a path or YAML text.  Texture paths resolve against `texture_root`
    (default: the current working directory, as image::open does)."""
    from . import _host

    try:
        if isinstance(source, os.PathLike) or (isinstance(source, str) and "\n" not in source
                                               and Path(source).exists()):
            loaded = _host.LoadedScene.from_file(source, texture_root)
        else:
            loaded = _host.LoadedScene.from_string(str(source), texture_root)
    except _host.HostError as e:
        raise SceneError(str(e)) from None
    try:
        return _scene_from_desc(loaded)
    finally:
        loaded.close()


_SURFACES = {_abi.SURFACE_DIFFUSE: "Diffuse", _abi.SURFACE_REFLECTING: "Reflecting",
             _abi.SURFACE_REFRACTIVE: "Refractive"}


def _scene_from_desc(loaded) -> "Scene":
    d = loaded.desc
    textures = []
    for i in range(d.n_textures):
        t = d.textures[i]
        img = np.ctypeslib.as_array(t.rgba, shape=(t.height * t.width * 4,)).copy().reshape(t.height, t.width, 4)
        textures.append((loaded.texture_path(i), img))

    def material(m) -> Material:
        if m.coloration == _abi.COLORATION_TEXTURE:
            path, img = textures[m.texture]
            col: Union[Color, Texture] = Texture(path, img, m.x_offset, m.y_offset)
        else:
            col = Color(*m.color)
        return Material(col, m.albedo, _SURFACES[m.surface], m.reflectivity, m.index, m.transparency)

    bodies: List[Body] = []
    for i in range(d.n_bodies):
        b = d.bodies[i]
        p = tuple(b.p)
        mat = material(b.material)
        if b.kind == _abi.BODY_SPHERE:
            bodies.append(Sphere(p[0:3], p[3], mat))
        elif b.kind == _abi.BODY_PLANE:
            bodies.append(Plane(p[0:3], p[3:6], mat))
        elif b.kind == _abi.BODY_DISK:
            bodies.append(Disk(p[0:3], p[3:6], p[6], mat))
        else:
            bodies.append(AABB((p[0:3], p[3:6]), mat))
    lights: List[Light] = []
    for i in range(d.n_lights):
        l = d.lights[i]
        cls = DirectionalLight if l.kind == _abi.LIGHT_DIRECTIONAL else SphericalLight
        lights.append(cls(tuple(l.v), Color(*l.color), l.intensity))
    return Scene(d.fov, Color(*d.default_color), d.max_recursion_depth, bodies, lights)


# ---------------------------------------------------------------- flat descriptor
class SceneDesc:
    """Owns the ctypes arrays behind an rg_scene_desc (pass `.desc` to the ABI)."""

    def __init__(self, scene: "Scene"):
        nb, nl = len(scene.bodies), len(scene.lights)
        self.bodies = (_abi.rg_body * max(nb, 1))()
        self.lights = (_abi.rg_light * max(nl, 1))()
        tex_index: dict = {}
        self._images: List[np.ndarray] = []
        for i, b in enumerate(scene.bodies):
            rb = self.bodies[i]
            if isinstance(b, Sphere):
                rb.kind, p = _abi.BODY_SPHERE, [*b.center, b.radius]
            elif isinstance(b, Plane):
                rb.kind, p = _abi.BODY_PLANE, [*b.origin, *b.normal]
            elif isinstance(b, Disk):
                rb.kind, p = _abi.BODY_DISK, [*b.origin, *b.normal, b.radius]
            elif isinstance(b, AABB):
                rb.kind, p = _abi.BODY_AABB, [*b.bounds[0], *b.bounds[1]]
            else:
                raise TypeError(f"not a body: {b!r}")
            for k, v in enumerate(p):
                rb.p[k] = v
            m = b.material
            rm = rb.material
            if isinstance(m.coloration, Texture):
                key = id(m.coloration.image)
                if key not in tex_index:
                    tex_index[key] = len(self._images)
                    self._images.append(np.ascontiguousarray(m.coloration.image, dtype=np.uint8))
                rm.coloration = _abi.COLORATION_TEXTURE
                rm.texture = tex_index[key]
                rm.x_offset = m.coloration.x_offset
                rm.y_offset = m.coloration.y_offset
            else:
                rm.coloration = _abi.COLORATION_COLOR
                rm.color[:] = [float(m.coloration.red), float(m.coloration.green), float(m.coloration.blue)]
                rm.texture = -1
            rm.albedo = m.albedo
            rm.surface = {"Diffuse": _abi.SURFACE_DIFFUSE, "Reflecting": _abi.SURFACE_REFLECTING,
                          "Refractive": _abi.SURFACE_REFRACTIVE}[m.surface]
            rm.reflectivity = m.reflectivity
            rm.index = m.index
            rm.transparency = m.transparency
        for i, l in enumerate(scene.lights):
            rl = self.lights[i]
            if isinstance(l, DirectionalLight):
                rl.kind, v = _abi.LIGHT_DIRECTIONAL, l.direction
            else:
                rl.kind, v = _abi.LIGHT_SPHERICAL, l.position
            rl.v[:] = list(v)
            rl.color[:] = [float(l.color.red), float(l.color.green), float(l.color.blue)]
            rl.intensity = l.intensity
        self.textures = (_abi.rg_texture * max(len(self._images), 1))()
        for i, im in enumerate(self._images):
            self.textures[i].height, self.textures[i].width = im.shape[0], im.shape[1]
            self.textures[i].rgba = im.ctypes.data_as(C.POINTER(C.c_uint8))
        d = _abi.rg_scene_desc()
        d.fov = scene.fov
        d.default_color[:] = [float(scene.default_color.red), float(scene.default_color.green),
                              float(scene.default_color.blue)]
        d.max_recursion_depth = scene.max_recursion_depth
        d.n_bodies, d.bodies = nb, C.cast(self.bodies, C.POINTER(_abi.rg_body))
        d.n_lights, d.lights = nl, C.cast(self.lights, C.POINTER(_abi.rg_light))
        d.n_textures, d.textures = len(self._images), C.cast(self.textures, C.POINTER(_abi.rg_texture))
        self.desc = d

    def ptr(self):
        return C.byref(self.desc)


# ---------------------------------------------------------------- device scene
class DeviceScene:
    """An rg_scene handle: the scene uploaded to one GPU."""

    def __init__(self, scene: "Scene", device: int = 0, path: Optional[int] = None, bvh: Optional[bool] = None):
        self._desc = SceneDesc(scene)
        h = C.c_void_p()
        _abi.check(_abi.lib().rg_scene_create(self._desc.ptr(), int(device), C.byref(h)), "rg_scene_create")
        self.handle = h
        self.device = device
        if path is not None:
            self.set_path(path)
        if bvh is not None:
            self.set_bvh(bvh)
        if getattr(scene, "lens", None) is not None:  # Scene.set_lens
            self.set_lens(scene.lens)
        if getattr(scene, "light_radii", None) is not None:  # Scene.set_light_radii
            self.set_light_radii(scene.light_radii)

    def close(self) -> None:
        if getattr(self, "handle", None):
            _abi.lib().rg_scene_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_path(self, path: int) -> None:
        """Force a kernel path (_abi.PATH_AUTO / PATH_LIGHT / PATH_HEAVY; include/raingun_debug.h)."""
        _abi.check(_abi.lib().rg_debug_set_path(self.handle, int(path)))

    def set_bvh(self, enable: bool) -> None:
        """Use (default) or bypass the sphere BVH (include/raingun_debug.h)."""
        _abi.check(_abi.lib().rg_debug_set_bvh(self.handle, 1 if enable else 0))

    def set_lightbuf(self, enable: bool) -> None:
        """Shadow rays test their light buffer cell's spheres (default) or walk the BVH (include/raingun_debug.h)."""
        _abi.check(_abi.lib().rg_debug_set_lightbuf(self.handle, 1 if enable else 0))

    def lightbuf_count(self) -> int:
        """Lights with a shadow-ray light buffer in use (include/raingun_debug.h)."""
        return int(_abi.lib().rg_debug_lightbuf_count(self.handle))

    def set_tile_order(self, mode) -> None:
        """Tile scheduling: True/1 probe-ordered, False/0 raster, -1 auto (include/raingun_debug.h)."""
        _abi.check(_abi.lib().rg_debug_set_tile_order(self.handle, int(mode)))

    def set_lane_depth(self, min_depth: int) -> None:
        """Rays at recursion depth >= min_depth walk the BVH per lane (0: all
        non-primary rays, large: none, -1: default) (include/raingun_debug.h)."""
        _abi.check(_abi.lib().rg_debug_set_lane_depth(self.handle, int(min_depth)))

    def set_image_bands(self, bands: int) -> None:
        """Row bands of host-visible renders (0: by frame size; include/raingun_debug.h)."""
        _abi.check(_abi.lib().rg_debug_set_image_bands(self.handle, int(bands)))

    def set_multi(self, mode: int = 0, stand_in: bool = False, bands: int = 0, only_rank: int = -1) -> None:
        """rg_render_multi delivery (raingun_debug.h): 0 per-device copies to the host, 1 RCCL gather;
        stand_in: every device is this one (ngpus > 1 on one GPU); only_rank: rehearse one device's work."""
        _abi.check(_abi.lib().rg_debug_set_multi(self.handle, int(mode), 1 if stand_in else 0, int(bands),
                                                 int(only_rank)))

    def set_host_ring(self, flush_small: int = -1, group_small: int = -1, flush_big: int = -1, group_big: int = -1,
                      multi_light_one: int = -1) -> None:
        """Light-path host frames: LDS-ring flush size and queue group of small / big launches,
        rg_render_multi's one launch per device for light scenes; -1 keeps a setting
        (include/raingun_debug.h rg_debug_set_host_ring)."""
        _abi.check(_abi.lib().rg_debug_set_host_ring(self.handle, int(flush_small), int(group_small), int(flush_big),
                                                     int(group_big), int(multi_light_one)))

    def set_host_split(self, pct: int) -> None:
        """Image bands -2 (split host frames): percent of the rows rendered into device
        memory and copied by DMA beside the one-launch rest; 0 = default (raingun_debug.h)."""
        _abi.check(_abi.lib().rg_debug_set_host_split(self.handle, int(pct)))

    def set_host_tile_shape(self, tile_wlog: int) -> None:
        """Tile shape of one-launch host-visible renders: log2 of the tile width, 3 (8x8) .. 6 (64x1);
        0 = automatic (16x4 for heavy-path scenes, 64x1 for light-path scenes)."""
        _abi.check(_abi.lib().rg_debug_set_host_tile_shape(self.handle, int(tile_wlog)))

    def last_plain(self) -> bool:
        """Did the latest render launch run a PLAIN light kernel (include/raingun_debug.h rg_debug_last_plain)?"""
        plain = C.c_int32(-1)
        _abi.check(_abi.lib().rg_debug_last_plain(self.handle, C.byref(plain)))
        return plain.value == 1

    def set_shadow_volume(self, on: bool) -> None:
        """False: launches pass no shadow mask volume, so the PLAIN light kernels test every body
        (include/raingun_debug.h rg_debug_set_shadow_volume)."""
        _abi.check(_abi.lib().rg_debug_set_shadow_volume(self.handle, 1 if on else 0))

    def shadow_volume_info(self) -> dict:
        """rg_debug_shadow_volume_info: built, enabled, g, bytes, build_ms, set_share."""
        info = _abi.rg_shadow_volume_info()
        _abi.check(_abi.lib().rg_debug_shadow_volume_info(self.handle, C.byref(info)))
        return {"built": bool(info.built), "enabled": bool(info.enabled), "g": info.g, "bytes": info.bytes,
                "build_ms": info.build_ms, "set_share": info.set_share}

    def last_shadow_volume(self) -> bool:
        """Did the latest render launch run a PLAIN light kernel with the shadow mask volume?"""
        used = C.c_int32(-1)
        _abi.check(_abi.lib().rg_debug_last_shadow_volume(self.handle, C.byref(used)))
        return used.value == 1

    def set_first_hit_tiles(self, on: bool) -> None:
        """False: no tile takes the PLAIN light kernels' first-hit path; every tile goes through the
        general state machine (include/raingun_debug.h rg_debug_set_first_hit_tiles)."""
        _abi.check(_abi.lib().rg_debug_set_first_hit_tiles(self.handle, 1 if on else 0))

    def last_first_hit_tiles(self) -> int:
        """Tiles of the latest render launch that finished on the PLAIN light kernels' first-hit path."""
        tiles = C.c_uint64(0)
        _abi.check(_abi.lib().rg_debug_last_first_hit_tiles(self.handle, C.byref(tiles)))
        return int(tiles.value)

    def set_exact_div(self, enable: bool) -> None:
        """False: launches behave as if the PLAIN kernels' camera-quotient check had failed, so they run
        the general kernel (include/raingun_debug.h rg_debug_set_exact_div)."""
        _abi.check(_abi.lib().rg_debug_set_exact_div(self.handle, 1 if enable else 0))

    def camera_check(self, width: int, height: int, fov: float):
        """rg_debug_camera_check: (pixels whose camera direction differs between the general and the
        PLAIN kernels' arithmetic, whether the launcher's checks admit that frame)."""
        bad, admitted = C.c_uint64(0), C.c_int32(-1)
        _abi.check(_abi.lib().rg_debug_camera_check(self.handle, int(width), int(height), float(fov), C.byref(bad),
                                                    C.byref(admitted)))
        return int(bad.value), admitted.value == 1

    def unscaled_check(self, op: int, a, b=None) -> int:
        """rg_debug_unscaled_check: the operands (float64 arrays; b for op 2, a / b) for which the PLAIN
        kernels' guarded sqrt (op 0), 1 / a (1), a / b (2) or sqrt and 1 / sqrt (3) differ from the
        compiler's operations in any bit."""
        import numpy as np

        a = np.ascontiguousarray(a, dtype=np.float64)
        bp = None
        if b is not None:
            b = np.ascontiguousarray(b, dtype=np.float64)
            assert b.shape == a.shape
            bp = b.ctypes.data_as(C.c_void_p)
        bad = C.c_uint64(0)
        _abi.check(_abi.lib().rg_debug_unscaled_check(self.handle, int(op), a.ctypes.data_as(C.c_void_p), bp, a.size,
                                                      C.byref(bad)))
        return int(bad.value)

    def bvh_info(self) -> _abi.rg_bvh_info:
        info = _abi.rg_bvh_info()
        _abi.check(_abi.lib().rg_debug_bvh_info(self.handle, C.byref(info)))
        return info

    def set_max_depth(self, depth: int) -> None:
        _abi.check(_abi.lib().rg_scene_set_max_depth(self.handle, int(depth)))

    def set_camera(self, camera: Optional[Camera]) -> None:
        """rg_scene_set_camera: the camera of every later render of this scene (raingun_amd/camera.py);
        None restores the reference's view from the origin down -z.  Launches already enqueued keep
        the camera they were enqueued with."""
        if camera is None:
            _abi.check(_abi.lib().rg_scene_set_camera(self.handle, None), "rg_scene_set_camera")
            return
        c = _abi.rg_camera((C.c_double * 3)(*camera.eye), (C.c_double * 3)(*camera.right),
                           (C.c_double * 3)(*camera.up), (C.c_double * 3)(*camera.forward))
        _abi.check(_abi.lib().rg_scene_set_camera(self.handle, C.byref(c)), "rg_scene_set_camera")

    def set_lens(self, lens: Optional[Lens]) -> None:
        """rg_scene_set_lens: the thin lens of every later render_image_aa / render_aa_async with
        samples >= 2 (raingun_amd/camera.py Lens); None, or an aperture of 0, is the pinhole again.
        One-ray-per-pixel renders ignore it, the adaptive ones are refused while it is set.  Launches
        already enqueued keep the lens they were enqueued with."""
        if lens is None:
            _abi.check(_abi.lib().rg_scene_set_lens(self.handle, None), "rg_scene_set_lens")
            return
        l = _abi.rg_lens(float(lens.aperture), float(lens.focus))
        _abi.check(_abi.lib().rg_scene_set_lens(self.handle, C.byref(l)), "rg_scene_set_lens")

    def set_light_radii(self, radii: Optional[Sequence[float]]) -> None:
        """rg_scene_set_light_radii: one radius (world units) per light, in the scene's order, for every later
        render_image_aa / render_aa_async with samples >= 2 -- soft shadows; a directional light's must be 0.
        None, or every radius 0: point lights again.  One-ray-per-pixel renders ignore them, the adaptive
        ones are refused while one is > 0.  Blocking: the call waits for the device to go idle before it
        rewrites the scene's table, and launches enqueued later see the new radii."""
        if radii is None:
            _abi.check(_abi.lib().rg_scene_set_light_radii(self.handle, None, 0), "rg_scene_set_light_radii")
            return
        r = [float(x) for x in radii]
        _abi.check(_abi.lib().rg_scene_set_light_radii(self.handle, (C.c_double * max(len(r), 1))(*r), len(r)),
                   "rg_scene_set_light_radii")

    def render_image(self, width: int, height: int, stats: Optional[_abi.rg_stats] = None,
                     out: Optional[np.ndarray] = None) -> np.ndarray:
        """rendering::render_image (rendering.rs:24-38) into host memory.  `out`
        (optional, (height, width, 4) uint8, C-contiguous) may be a buffer
        registered with register_host() for direct DMA."""
        if out is None:
            out = np.empty((height, width, 4), dtype=np.uint8)
        assert out.shape == (height, width, 4) and out.dtype == np.uint8 and out.flags.c_contiguous
        st = stats if stats is not None else _abi.rg_stats()
        _abi.check(_abi.lib().rg_render_image(self.handle, width, height, out.ctypes.data, C.byref(st)),
                   "rg_render_image")
        return out

    def render_image_aa(self, width: int, height: int, samples: int, want_rgb: bool = False,
                        stats: Optional[_abi.rg_stats] = None, out: Optional[np.ndarray] = None):
        """rg_render_image_aa: render_image with samples x samples rays per pixel on the regular
        sub-pixel grid, box-filtered (raingun_amd/aa.py states the arithmetic).  Returns the
        (height, width, 4) uint8 frame, or (frame, (height, width, 3) float32 means) with want_rgb."""
        if out is None:
            out = np.empty((height, width, 4), dtype=np.uint8)
        assert out.shape == (height, width, 4) and out.dtype == np.uint8 and out.flags.c_contiguous
        rgb = np.empty((height, width, 3), dtype=np.float32) if want_rgb else None
        st = stats if stats is not None else _abi.rg_stats()
        _abi.check(_abi.lib().rg_render_image_aa(self.handle, width, height, int(samples), out.ctypes.data,
                                                 rgb.ctypes.data if rgb is not None else None, C.byref(st)),
                   "rg_render_image_aa")
        return (out, rgb) if want_rgb else out

    def render_image_aa_adaptive(self, width: int, height: int, samples: int, threshold: int, want_rgb: bool = False,
                                 want_mask: bool = False, stats: Optional[_abi.rg_stats] = None,
                                 out: Optional[np.ndarray] = None):
        """rg_render_image_aa_adaptive: render_image_aa that traces the samples x samples rays only of the
        pixels whose 8-neighbourhood contrast in the 1-sample frame is >= threshold (0..256;
        raingun_amd/aa.py resolve_adaptive states the result).  Returns the (height, width, 4) uint8
        frame, followed by the (height, width, 3) float32 means with want_rgb and by the
        (height, width) uint8 mask (1 = supersampled) with want_mask."""
        if out is None:
            out = np.empty((height, width, 4), dtype=np.uint8)
        assert out.shape == (height, width, 4) and out.dtype == np.uint8 and out.flags.c_contiguous
        rgb = np.empty((height, width, 3), dtype=np.float32) if want_rgb else None
        mask = np.empty((height, width), dtype=np.uint8) if want_mask else None
        st = stats if stats is not None else _abi.rg_stats()
        _abi.check(_abi.lib().rg_render_image_aa_adaptive(
            self.handle, width, height, int(samples), int(threshold), out.ctypes.data,
            rgb.ctypes.data if rgb is not None else None, mask.ctypes.data if mask is not None else None,
            C.byref(st)), "rg_render_image_aa_adaptive")
        res = (out,) + ((rgb,) if want_rgb else ()) + ((mask,) if want_mask else ())
        return res if len(res) > 1 else out

    def edge_mask(self, rgba: np.ndarray, threshold: int):
        """rg_edge_mask on this scene's device: (H, W, 4) uint8 RGBA -> ((H, W) uint8 mask, its number
        of ones), as aa.edge_mask computes it."""
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        if rgba.ndim != 3 or rgba.shape[2] != 4 or rgba.size == 0:
            raise ValueError("expected (height, width, 4) uint8 RGBA")
        h, w = rgba.shape[:2]
        mask = np.empty((h, w), dtype=np.uint8)
        n = C.c_uint32(0)
        _abi.check(_abi.lib().rg_edge_mask(int(self.device), rgba.ctypes.data, w, h, int(threshold), mask.ctypes.data,
                                           C.byref(n)), "rg_edge_mask")
        return mask, int(n.value)

    def resolve_box(self, rgb: np.ndarray, samples: int):
        """rg_resolve_box on this scene's device: (samples*H, samples*W, 3) float32 samples ->
        ((H, W, 3) float32 means, (H, W, 4) uint8 RGBA), as aa.resolve_box computes them."""
        k = int(samples)
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        if rgb.ndim != 3 or rgb.shape[2] != 3 or k < 1 or rgb.shape[0] % k or rgb.shape[1] % k:
            raise ValueError("expected (samples*height, samples*width, 3) float32 samples")
        h, w = rgb.shape[0] // k, rgb.shape[1] // k
        mean = np.empty((h, w, 3), dtype=np.float32)
        rgba = np.empty((h, w, 4), dtype=np.uint8)
        _abi.check(_abi.lib().rg_resolve_box(int(self.device), rgb.ctypes.data, w, h, k, rgba.ctypes.data,
                                             mean.ctypes.data), "rg_resolve_box")
        return mean, rgba

    def set_aa_band_rows(self, rows: int) -> None:
        """Output rows per band of supersampled renders (0: automatic; include/raingun_debug.h)."""
        _abi.check(_abi.lib().rg_debug_set_aa_band_rows(self.handle, int(rows)))

    def render_multi(self, width: int, height: int, ngpus: int, tile_rows: int = 0,
                     stats: Optional[_abi.rg_stats] = None, out: Optional[np.ndarray] = None) -> np.ndarray:
        """rg_render_multi: the frame over `ngpus` devices of this process (row
        tiles, one RCCL gather to this scene's device), delivered to host memory."""
        if out is None:
            out = np.empty((height, width, 4), dtype=np.uint8)
        st = stats if stats is not None else _abi.rg_stats()
        _abi.check(_abi.lib().rg_render_multi(self.handle, width, height, int(ngpus), int(tile_rows),
                                              out.ctypes.data, C.byref(st)), "rg_render_multi")
        return out

    def render_stream(self, width: int, height: int, on_tile, tile_rows: int = 16,
                      stats: Optional[_abi.rg_stats] = None) -> int:
        """rg_render_stream: on_tile(row0, band) gets each band of finished RGBA8
        rows (a copy); return True to cancel.  Returns the rg_status."""
        st = stats if stats is not None else _abi.rg_stats()

        def cb(row0, rows, w, ptr, _user):
            band = np.ctypeslib.as_array(ptr, shape=(rows * w * 4,)).reshape(rows, w, 4).copy()
            return 1 if on_tile(int(row0), band) else 0

        fn = _abi.TILE_CALLBACK(cb)
        return _abi.lib().rg_render_stream(self.handle, width, height, tile_rows, fn, None, C.byref(st))

    def stream_status(self, stream: int):
        """(status, error_pixel) of the launches on `stream` (a hipStream_t value) since the last call."""
        px = C.c_int32(-1)
        st = _abi.lib().rg_stream_status(self.handle, C.c_void_p(stream), C.byref(px))
        return st, px.value

    def release_stream(self, stream: int) -> None:
        _abi.check(_abi.lib().rg_scene_release_stream(self.handle, C.c_void_p(stream)), "rg_scene_release_stream")

    def render_tiles(self, width: int, height: int, tile_rows: int = 0, stride: int = 1, offset: int = 0,
                     want_rgb: bool = False, stats: Optional[_abi.rg_stats] = None):
        t = _abi.rg_tiling(tile_rows or height, stride, offset)
        rows = _abi.lib().rg_tiling_rows(height, C.byref(t))
        rgba = np.empty((rows, width, 4), dtype=np.uint8)
        rgb = np.empty((rows, width, 3), dtype=np.float32) if want_rgb else None
        st = stats if stats is not None else _abi.rg_stats()
        status = _abi.lib().rg_render_tiles(self.handle, width, height, C.byref(t), rgba.ctypes.data,
                                            rgb.ctypes.data if rgb is not None else None, C.byref(st))
        _abi.check(status, "rg_render_tiles")
        return (rgba, rgb) if want_rgb else rgba

    def render_aov(self, width: int, height: int, layers=aov.LAYERS, stats: Optional[_abi.rg_stats] = None) -> dict:
        """rg_render_aov: the AOV layers of the frame rg_render_image renders (raingun_amd/aov.py), one
        primary ray per pixel through the scene's camera.  Returns {layer name: numpy array}.  A device
        error (the reference's panics) raises RaingunError, as render_image does; `stats` then names
        the first failing pixel."""
        layers = aov.parse_layers(layers)
        out = {n: np.empty(aov.layer_shape(n, height, width), dtype=aov.DTYPES[n]) for n in layers}
        v = _abi.rg_aov(**{n: out[n].ctypes.data for n in layers})
        st = stats if stats is not None else _abi.rg_stats()
        _abi.check(_abi.lib().rg_render_aov(self.handle, width, height, C.byref(v), C.byref(st)), "rg_render_aov")
        return out

    def render_aov_tiles(self, width: int, height: int, tile_rows: int = 0, stride: int = 1, offset: int = 0,
                         layers=aov.LAYERS, stream: int = 0, stats: Optional[_abi.rg_stats] = None,
                         out: Optional[dict] = None) -> dict:
        """rg_render_aov_async: the layers of the tiles a tiling selects (render_tiles' packing), in
        device memory, enqueued on `stream` (a hipStream_t value).  Returns {layer name: torch tensor on
        this scene's device}; `out` supplies the tensors to write into.  Asynchronous unless `stats` is
        given: the caller synchronises `stream` before reading the tensors."""
        import torch

        layers = aov.parse_layers(layers)
        t = _abi.rg_tiling(tile_rows or height, stride, offset)
        rows = _abi.lib().rg_tiling_rows(height, C.byref(t))
        dev = torch.device("cuda", self.device)
        if out is None:
            tt = {np.int32: torch.int32, np.float64: torch.float64, np.float32: torch.float32}
            out = {n: torch.empty(aov.layer_shape(n, rows, width), dtype=tt[aov.DTYPES[n]], device=dev) for n in layers}
        for n in layers:
            assert tuple(out[n].shape) == aov.layer_shape(n, rows, width) and out[n].is_contiguous(), n
        v = _abi.rg_aov(**{n: out[n].data_ptr() for n in layers})
        status = _abi.lib().rg_render_aov_async(self.handle, width, height, C.byref(t), C.byref(v), C.c_void_p(stream),
                                                C.byref(stats) if stats is not None else None)
        _abi.check(status, "rg_render_aov_async")
        return out

    def render_ao(self, width: int, height: int, samples: int, radius: float = float("inf"), bias: float = 1e-13,
                  stats: Optional[_abi.rg_stats] = None) -> np.ndarray:
        """rg_render_ao: the ambient occlusion of the frame render_aov renders (raingun_amd/ao.py) -- per hit pixel
        samples x samples any-hit rays over the hemisphere above the primary hit, the open share as float32;
        1.0 on a miss.  Returns an (H, W) float32 array.  A device error (the reference's panics) raises
        RaingunError, as render_image does; `stats` then names the first failing pixel."""
        out = np.empty((height, width), dtype=np.float32)
        v = _abi.rg_ao(int(samples), 0, float(radius), float(bias))
        st = stats if stats is not None else _abi.rg_stats()
        _abi.check(_abi.lib().rg_render_ao(self.handle, width, height, C.byref(v), out.ctypes.data, C.byref(st)),
                   "rg_render_ao")
        return out

    def render_ao_tiles(self, width: int, height: int, samples: int, radius: float = float("inf"), bias: float = 1e-13,
                        tile_rows: int = 0, stride: int = 1, offset: int = 0, stream: int = 0,
                        stats: Optional[_abi.rg_stats] = None, out=None):
        """rg_render_ao_async: the ambient occlusion of the tiles a tiling selects (render_tiles' packing), in
        device memory, enqueued on `stream` (a hipStream_t value).  Returns a (rows, W) float32 torch tensor on
        this scene's device; `out` supplies the tensor to write into.  Asynchronous unless `stats` is given:
        the caller synchronises `stream` before reading the tensor."""
        import torch

        t = _abi.rg_tiling(tile_rows or height, stride, offset)
        rows = _abi.lib().rg_tiling_rows(height, C.byref(t))
        if out is None:
            out = torch.empty((rows, width), dtype=torch.float32, device=torch.device("cuda", self.device))
        assert tuple(out.shape) == (rows, width) and out.dtype == torch.float32 and out.is_contiguous()
        v = _abi.rg_ao(int(samples), 0, float(radius), float(bias))
        status = _abi.lib().rg_render_ao_async(self.handle, width, height, C.byref(t), C.byref(v), C.c_void_p(out.data_ptr()),
                                               C.c_void_p(stream), C.byref(stats) if stats is not None else None)
        _abi.check(status, "rg_render_ao_async")
        return out

    def filter_ao(self, ao_in: np.ndarray, body: np.ndarray, normal: np.ndarray, radius: int = 2,
                  normal_min: float = 0.9) -> np.ndarray:
        """rg_ao_filter on this scene's device: the edge-stopping tent filter of an AO pass, guided by the AOV
        pass's body and normal layers (raingun_amd/ambient.py filter_ao states it).  (H, W) float32, (H, W)
        int32, (H, W, 3) float32 -> (H, W) float32; any shape."""
        a = np.ascontiguousarray(ao_in, dtype=np.float32)
        b = np.ascontiguousarray(body, dtype=np.int32)
        n = np.ascontiguousarray(normal, dtype=np.float32)
        if a.ndim != 2 or a.size == 0 or b.shape != a.shape or n.shape != (*a.shape, 3):
            raise ValueError("expected ao (H, W), body (H, W) and normal (H, W, 3)")
        h, w = a.shape
        out = np.empty((h, w), dtype=np.float32)
        f = _abi.rg_ao_filter_desc(int(radius), float(normal_min))
        _abi.check(_abi.lib().rg_ao_filter(int(self.device), a.ctypes.data, b.ctypes.data, n.ctypes.data, w, h,
                                           C.byref(f), out.ctypes.data), "rg_ao_filter")
        return out

    def render_ambient(self, width: int, height: int, color, ao_samples: int, ao_radius: float = float("inf"),
                       ao_bias: float = 1e-13, samples: int = 1, filter_radius: int = 2, normal_min: float = 0.9,
                       want_rgb: bool = False, want_ao: bool = False, stats: Optional[_abi.rg_stats] = None):
        """rg_render_image_ambient: the samples x samples supersampled frame plus an ambient light of `color`
        (three floats, or one for grey) weighted by the filtered AO pass (raingun_amd/ambient.py states the
        filter and the compose).  filter_radius 0: the raw pass.  Returns the (H, W, 4) uint8 frame, followed by
        the (H, W, 3) float32 composed colours with want_rgb and by the (H, W) float32 filtered pass with
        want_ao.  A device error raises RaingunError; `stats` then names the first failing pixel."""
        col = np.broadcast_to(np.asarray(color, dtype=np.float32).reshape(-1), (3,))
        out = np.empty((height, width, 4), dtype=np.uint8)
        rgb = np.empty((height, width, 3), dtype=np.float32) if want_rgb else None
        aof = np.empty((height, width), dtype=np.float32) if want_ao else None
        m = _abi.rg_ambient((C.c_float * 3)(*[float(c) for c in col]), int(samples),
                            _abi.rg_ao(int(ao_samples), 0, float(ao_radius), float(ao_bias)), int(filter_radius),
                            float(normal_min))
        st = stats if stats is not None else _abi.rg_stats()
        _abi.check(_abi.lib().rg_render_image_ambient(
            self.handle, width, height, C.byref(m), out.ctypes.data, rgb.ctypes.data if rgb is not None else None,
            aof.ctypes.data if aof is not None else None, C.byref(st)), "rg_render_image_ambient")
        res = (out,) + ((rgb,) if want_rgb else ()) + ((aof,) if want_ao else ())
        return res if len(res) > 1 else out

    def trace(self, rays: np.ndarray):
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        n = rays.shape[0]
        dist = np.empty(n, dtype=np.float64)
        body = np.empty(n, dtype=np.int32)
        _abi.check(_abi.lib().rg_trace(self.handle, rays.ctypes.data, n, dist.ctypes.data, body.ctypes.data),
                   "rg_trace")
        return dist, body


# ---------------------------------------------------------------- Scene
@dataclass
class Scene:                   # scene.rs:11-31
    fov: float = 90.0
    default_color: Color = field(default_factory=Color.black)
    max_recursion_depth: int = 10
    bodies: List[Body] = field(default_factory=list)
    lights: List[Light] = field(default_factory=list)

    from_yaml = staticmethod(load_scene)
    lens = None  # set_lens: not a field of the scene file (scene.rs has no lens), so not a dataclass field

    def set_lens(self, lens: Optional[Lens]) -> None:
        """The thin lens (raingun_amd/camera.py Lens) that every DeviceScene made of this scene from now on
        starts with, and so render_image(samples >= 2); None: the pinhole."""
        self.lens = lens

    light_radii = None  # set_light_radii: not a field of the scene file either

    def set_light_radii(self, radii: Optional[Sequence[float]]) -> None:
        """The lights' radii (DeviceScene.set_light_radii: one per light, in order) that every DeviceScene made
        of this scene from now on starts with, and so render_image(samples >= 2); None: point lights."""
        self.light_radii = None if radii is None else tuple(float(r) for r in radii)

    def to_device(self, device: int = 0) -> DeviceScene:
        return DeviceScene(self, device)

    # scene.rs:41-43 -> rendering::render_image (rendering.rs:24-38), on the GPU
    # samples > 1: samples x samples rays per pixel, box-filtered (rg_render_image_aa);
    # adaptive = T (0..256): only for pixels on edges of the 1-sample frame (rg_render_image_aa_adaptive)
    def render_image(self, width: int, height: int, device: int = 0, samples: int = 1,
                     adaptive: Optional[int] = None, camera: Optional[Camera] = None) -> np.ndarray:
        ds = DeviceScene(self, device)
        try:
            ds.set_camera(camera)
            if adaptive is not None:
                return ds.render_image_aa_adaptive(width, height, samples, adaptive)
            if samples != 1:
                return ds.render_image_aa(width, height, samples)
            return ds.render_image(width, height)
        finally:
            ds.close()

    # the AOV layers of render_image's frame (rg_render_aov; raingun_amd/aov.py): {layer name: numpy array}
    def render_aov(self, width: int, height: int, device: int = 0, layers=aov.LAYERS,
                   camera: Optional[Camera] = None) -> dict:
        ds = DeviceScene(self, device)
        try:
            ds.set_camera(camera)
            return ds.render_aov(width, height, layers)
        finally:
            ds.close()

    # the ambient occlusion of render_aov's frame (rg_render_ao; raingun_amd/ao.py): an (H, W) float32 array
    def render_ao(self, width: int, height: int, samples: int, radius: float = float("inf"), bias: float = 1e-13,
                  device: int = 0, camera: Optional[Camera] = None) -> np.ndarray:
        ds = DeviceScene(self, device)
        try:
            ds.set_camera(camera)
            return ds.render_ao(width, height, samples, radius, bias)
        finally:
            ds.close()

    # render_image's frame plus an ambient light weighted by the filtered AO pass (rg_render_image_ambient;
    # raingun_amd/ambient.py): the (H, W, 4) uint8 frame
    def render_ambient(self, width: int, height: int, color, ao_samples: int, ao_radius: float = float("inf"),
                       ao_bias: float = 1e-13, samples: int = 1, filter_radius: int = 2, normal_min: float = 0.9,
                       device: int = 0, camera: Optional[Camera] = None) -> np.ndarray:
        ds = DeviceScene(self, device)
        try:
            ds.set_camera(camera)
            return ds.render_ambient(width, height, color, ao_samples, ao_radius, ao_bias, samples, filter_radius,
                                     normal_min)
        finally:
            ds.close()

    # scene.rs:45-51 -> rendering::render_image_stream (rendering.rs:40-69).  The
    # reference sends one RenderedPixel per pixel; here the callback receives
    # bands of `tile_rows` finished RGBA8 rows.  Return True from it to cancel.
    def streaming_render(self, width: int, height: int,
                         on_tile: Callable[[int, np.ndarray], Optional[bool]],
                         tile_rows: int = 16, device: int = 0, camera: Optional[Camera] = None) -> _abi.rg_stats:
        ds = DeviceScene(self, device)
        stats = _abi.rg_stats()
        try:
            ds.set_camera(camera)
            _abi.check(ds.render_stream(width, height, on_tile, tile_rows, stats), "rg_render_stream")
        finally:
            ds.close()
        return stats

    # scene.rs:34-39
    def trace(self, origin: Sequence[float], direction: Sequence[float], device: int = 0):
        ds = DeviceScene(self, device)
        try:
            dist, body = ds.trace(np.array([*origin, *direction], dtype=np.float64))
        finally:
            ds.close()
        if body[0] < 0:
            return None
        return float(dist[0]), int(body[0])
