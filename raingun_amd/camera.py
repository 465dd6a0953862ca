"""The movable camera (include/raingun.h rg_camera; raingun_amd/csrc/rg_camera.h states the arithmetic),
and the thin lens (Lens) that supersampled frames may look through.

A camera is eye, right, up, forward: four triples of doubles.  The primary ray of pixel (x, y) leaves
`eye` towards normalize((right * sx + up * sy) + forward), with sx, sy the reference's sensor
coordinates (ray.rs:43-51); Camera.identity() is the reference's view from the origin down -z.
look_at restates rg_camera_look_at in Python floats (the same IEEE doubles, the same order, no
fused operations), so it needs no library; tests/test_camera_cpu.py compares the two bit for bit.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

Vec = Tuple[float, float, float]


def _vec(v: Sequence[float]) -> Vec:
    v = tuple(float(c) for c in v)
    if len(v) != 3:
        raise ValueError("expected three numbers")
    return v  # type: ignore[return-value]


def _finite(v: Vec) -> bool:
    return all(math.isfinite(c) for c in v)


def _normalize(v: Vec) -> Vec:
    inv = 1.0 / math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return (v[0] * inv, v[1] * inv, v[2] * inv)


def _cross(a: Vec, b: Vec) -> Vec:
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


@dataclass(frozen=True)
class Camera:
    eye: Vec = (0.0, 0.0, 0.0)
    right: Vec = (1.0, 0.0, 0.0)
    up: Vec = (0.0, 1.0, 0.0)
    forward: Vec = (0.0, 0.0, -1.0)

    def __post_init__(self):
        for name in ("eye", "right", "up", "forward"):
            object.__setattr__(self, name, _vec(getattr(self, name)))
        if not self.valid():
            raise ValueError("a camera needs finite members and a non-zero forward")

    def valid(self) -> bool:
        return (_finite(self.eye) and _finite(self.right) and _finite(self.up) and _finite(self.forward)
                and any(c != 0.0 for c in self.forward))

    @staticmethod
    def identity() -> "Camera":
        """The reference's view (ray.rs:37-54): from the origin down -z."""
        return Camera()

    @staticmethod
    def at(eye: Sequence[float]) -> "Camera":
        """Looking down -z from `eye` (the CLI's --eye without --look-at)."""
        return Camera(eye=_vec(eye))

    @staticmethod
    def look_at(eye: Sequence[float], target: Sequence[float], up: Sequence[float] = (0.0, 1.0, 0.0)) -> "Camera":
        """forward = normalize(target - eye), right = normalize(cross(forward, up)), up = cross(right,
        forward).  ValueError for target == eye, a non-finite input, cross(forward, up) == 0 or a result
        that is no camera -- what rg_camera_look_at answers with RG_ERR_INVALID_ARGUMENT."""
        e, t, h = _vec(eye), _vec(target), _vec(up)
        if not (_finite(e) and _finite(t) and _finite(h)):
            raise ValueError("look_at: non-finite input")
        if t == e:
            raise ValueError("look_at: target == eye")
        f = _normalize((t[0] - e[0], t[1] - e[1], t[2] - e[2]))
        c = _cross(f, h)
        if c == (0.0, 0.0, 0.0):
            raise ValueError("look_at: the up hint is parallel to the view direction")
        r = _normalize(c)
        u = _cross(r, f)
        if not (_finite(r) and _finite(u) and _finite(f) and any(x != 0.0 for x in f)):
            raise ValueError("look_at: the result is no camera")
        return Camera(e, r, u, f)


@dataclass(frozen=True)
class Lens:
    """A thin lens (include/raingun.h rg_lens; raingun_amd/csrc/rg_lens.h states the arithmetic): depth of
    field for the supersampled frames (samples >= 2).  aperture: the lens radius in world units, 0 a
    pinhole; focus: the distance of the plane in focus along the camera's forward, in units of |forward|."""
    aperture: float
    focus: float

    def __post_init__(self):
        object.__setattr__(self, "aperture", float(self.aperture))
        object.__setattr__(self, "focus", float(self.focus))
        if not (math.isfinite(self.aperture) and math.isfinite(self.focus) and self.aperture >= 0.0 and self.focus > 0.0):
            raise ValueError("a lens needs a finite aperture >= 0 and a finite focus > 0")


def lens_from_flags(aperture, focus, samples: int, adaptive) -> "Optional[Lens]":
    """The lens of the CLI's --aperture R --focus D (each a string or None): None without either.
    ValueError unless both are given and are a lens, with --samples >= 2 and no --adaptive."""
    if aperture is None and focus is None:
        return None
    if aperture is None or focus is None:
        raise ValueError("--aperture and --focus go together")
    lens = Lens(float(aperture), float(focus))  # float('x') raises ValueError
    if samples < 2:
        raise ValueError("a lens needs --samples 2 or more")
    if adaptive is not None:
        raise ValueError("a lens cannot be combined with --adaptive")
    return lens


def light_radii_from_flags(text, samples: int, adaptive) -> "Optional[Tuple[float, ...]]":
    """The numbers of the CLI's --light-radius (a string or None) as given: one for every spherical light, or a
    comma list with one entry per light of the scene in YAML order (spread_light_radii, once the scene is
    read); None without the flag.  ValueError unless each is finite and >= 0, with --samples >= 2 and no
    --adaptive."""
    if text is None:
        return None
    radii = tuple(float(p) for p in str(text).split(","))  # float('x') raises ValueError
    if not all(math.isfinite(r) and r >= 0.0 for r in radii):
        raise ValueError("a light radius is a finite number >= 0")
    if samples < 2:
        raise ValueError("area lights need --samples 2 or more")
    if adaptive is not None:
        raise ValueError("area lights cannot be combined with --adaptive")
    return radii


def spread_light_radii(radii: Sequence[float], spherical: Sequence[bool]) -> Tuple[float, ...]:
    """--light-radius for a scene whose lights are spherical[l]: one number goes to every spherical light (a
    directional one gets 0), a list is one entry per light.  ValueError for a list of another length."""
    if len(radii) == 1:
        return tuple(radii[0] if s else 0.0 for s in spherical)
    if len(radii) != len(spherical):
        raise ValueError(f"--light-radius lists {len(radii)} radii, the scene has {len(spherical)} lights")
    return tuple(radii)


def parse_triple(text: str) -> Vec:
    """'X,Y,Z' -> three floats (the CLI's --eye / --look-at / --up); ValueError otherwise."""
    parts = text.split(",")
    if len(parts) != 3:
        raise ValueError(f"expected X,Y,Z, got {text!r}")
    v = tuple(float(p) for p in parts)  # float('') and float('x') raise ValueError
    if not _finite(v):  # type: ignore[arg-type]
        raise ValueError(f"non-finite component in {text!r}")
    return v  # type: ignore[return-value]


def camera_from_flags(eye, look_at, up):
    """The camera of the CLI's flags (each a parsed triple or None): None without --eye and
    --look-at; --eye alone looks down -z from the eye; --look-at from the origin if --eye is absent.
    ValueError for --up without --look-at and for a rejected look-at."""
    if eye is None and look_at is None:
        if up is not None:
            raise ValueError("--up needs --look-at")
        return None
    if look_at is None:
        if up is not None:
            raise ValueError("--up needs --look-at")
        return Camera.at(eye)
    return Camera.look_at(eye if eye is not None else (0.0, 0.0, 0.0), look_at, up if up is not None else (0.0, 1.0, 0.0))
