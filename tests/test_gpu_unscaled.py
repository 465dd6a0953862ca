"""The PLAIN light kernels' guarded unscaled f64 sqrt and division (rg_k_math.h
sqrt_guarded / rcp_guarded / div_guarded / sqrt_rcp_guarded, rg_exact.h's exponent window).  What
ships in the render kernels is sqrt_rcp_guarded in the spherical lights' setup alone; sphere_tail, the
planes' quotients, the sphere normal and fresnel / transmission stay the compiler's (the guarded
forms measured slower or no faster there).  Everything stays bit for bit:

  * rg_debug_unscaled_check runs all four guarded primitives on the device, fallback included, beside
    the compiler's sqrt and division: no operand differs -- random mantissas at every exponent of the
    window, both edges and a binade beyond each, powers of two, all-ones mantissas, perfect squares,
    quotient pairs at the extreme exponent differences, and the excluded classes (zeros, denormals,
    infinities, NaNs, negative sqrt operands), as whole waves of admitted operands, whole waves of
    refused ones and mixed waves;
  * frames equal the CPU restatement byte for byte with equal ray counts, and equal the general
    kernel's (rg_debug_set_exact_div(0)), as single and pipelined launches, and rg_debug_last_plain
    names the kernel in every case: test1; test1 scaled by 2^-100 and by 2^-300; a spherical light a
    few ulps off the plane it lights; small spheres; a refractive sphere around the camera and one
    seen from outside, indices 1.33 and 1/1.33; a plane parallel to the directional light and one
    facing it.  The first four bear on the lights' setup; the last three are the issue's scenes for
    groups that did not ship and guard the frames around it.
"""
import copy

import numpy as np
import pytest

import gpu_launch
from gpu_launch import SIZES, device_launch, oracle_frame, require_device
from raingun_amd import _abi
from raingun_amd.color import Color
from raingun_amd.scene import (DeviceScene, DirectionalLight, Material, Plane, Scene, Sphere,
                               SphericalLight)

pytestmark = pytest.mark.gpu

LO, HI = 767, 1279            # the window's biased exponents (rg_exact.h RG_UNSCALED_EXP_LO / _HI)
ONES = (1 << 52) - 1


@pytest.fixture(scope="module", autouse=True)
def _device():
    require_device()


# ---------------------------------------------------------------- the primitives, both ways
def _f64(sign, biased, mantissa):
    """float64 array from sign, biased exponent and mantissa arrays (broadcast)."""
    s, e, m = np.broadcast_arrays(np.asarray(sign, np.uint64), np.asarray(biased, np.uint64), np.asarray(mantissa, np.uint64))
    return ((s << np.uint64(63)) | (e << np.uint64(52)) | (m & np.uint64(ONES))).view(np.float64)


def _specials():
    """The excluded classes: zeros, denormals, the smallest normals, infinities, NaNs (quiet, with a
    payload, signalling), a few ordinary negatives, and the format's far ends."""
    bits = [0x0000000000000000, 0x8000000000000000, 0x0000000000000001, 0x8000000000000001, 0x000FFFFFFFFFFFFF,
            0x0008000000000000, 0x800FFFFFFFFFFFFF, 0x0010000000000000, 0x8010000000000000, 0x0010000000000001,
            0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000123,
            0x7FF0000000000001, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF, 0x7FE0000000000000, 0x0360000000000000,
            0x0350000000000000, 0x7FD0000000000000, 0x0020000000000000]
    neg = np.array([-1.0, -4.0, -2.0 ** -300, -2.0 ** 300, -1e-13, -0.3], dtype=np.float64)
    return np.concatenate([np.array(bits, dtype=np.uint64).view(np.float64), neg])


def _window_operands(rng, both_signs):
    """~2^16 operands for a one-operand primitive.  Laid out so that the device sees whole waves of
    admitted operands (the fallback is skipped), whole waves of refused ones, and mixed waves."""
    exps = np.arange(LO, HI + 1, dtype=np.uint64)
    inside = _f64(0, np.repeat(exps, 64), rng.integers(0, 1 << 52, size=exps.size * 64, dtype=np.uint64))  # 32,832: whole waves
    edges = np.concatenate([_f64(0, e, np.array([0, 1, ONES, ONES - 1, 1 << 51], dtype=np.uint64)) for e in (LO, HI)])
    pow2 = _f64(0, np.arange(1, 2047, dtype=np.uint64), 0)            # every normal power of two
    ones = _f64(0, np.arange(1, 2047, dtype=np.uint64), ONES)         # all-ones mantissas
    k = np.arange(1, 2049, dtype=np.float64)
    squares = np.concatenate([k * k, (k * k) * 2.0 ** -200, (k * k) * 2.0 ** 200, (k * k) * 2.0 ** -600])  # perfect squares
    beyond = np.concatenate([_f64(0, e, rng.integers(0, 1 << 52, size=64, dtype=np.uint64)) for e in (LO - 1, HI + 1)]
                            + [_f64(0, e, np.array([0, ONES], dtype=np.uint64)) for e in (LO - 1, HI + 1)])
    outside = _f64(0, rng.integers(1, LO - 1, size=1024, dtype=np.uint64), rng.integers(0, 1 << 52, size=1024, dtype=np.uint64))
    outside = np.concatenate([outside, _f64(0, rng.integers(HI + 2, 2047, size=1024, dtype=np.uint64),
                                            rng.integers(0, 1 << 52, size=1024, dtype=np.uint64))])
    spec = _specials()
    scattered = _f64(0, rng.integers(LO, HI + 1, size=16384, dtype=np.uint64), rng.integers(0, 1 << 52, size=16384, dtype=np.uint64))
    parts = [inside, scattered, edges, pow2, ones, squares, beyond, outside, spec]
    if both_signs:
        parts += [-inside[::8], -edges, -pow2[::4], -beyond]
    else:
        parts += [-inside[::64]]  # negative sqrt operands with admitted exponents: refused by the sign bit
    # mixed waves: one refused operand among 63 admitted ones, at every lane position once
    mixed = inside[:64 * 64].copy()
    for w in range(64):
        mixed[64 * w + w] = spec[w % spec.size]
    parts.append(mixed)
    a = np.concatenate(parts)
    assert inside.size % 64 == 0 and a.size >= 60000
    return a


def _quotient_operands(rng):
    """~2^16 (a, b) pairs: random admitted pairs of either sign, the extreme exponent differences of
    the window and a binade beyond, equal operands, and every excluded class on either side."""
    n = 48 * 1024
    ea, eb = rng.integers(LO, HI + 1, size=n, dtype=np.uint64), rng.integers(LO, HI + 1, size=n, dtype=np.uint64)
    a = _f64(rng.integers(0, 2, size=n, dtype=np.uint64), ea, rng.integers(0, 1 << 52, size=n, dtype=np.uint64))
    b = _f64(rng.integers(0, 2, size=n, dtype=np.uint64), eb, rng.integers(0, 1 << 52, size=n, dtype=np.uint64))
    A, B = [a], [b]
    mant = np.array([0, 1, ONES, ONES - 1, 1 << 51, 0x5555555555555, 0xAAAAAAAAAAAAA], dtype=np.uint64)
    ma, mb = [x.ravel() for x in np.meshgrid(mant, mant)]
    for xa, xb in ((HI, LO), (LO, HI), (HI, HI), (LO, LO), (HI + 1, LO), (LO - 1, HI), (HI, LO - 1), (LO, HI + 1), (1023, 1023)):
        for sa, sb in ((0, 0), (1, 0), (0, 1)):
            A.append(_f64(sa, xa, ma))
            B.append(_f64(sb, xb, mb))
    r = rng.integers(0, 1 << 52, size=4096, dtype=np.uint64)
    A.append(_f64(0, HI, r)); B.append(_f64(0, LO, r[::-1]))           # quotients up to 2^513
    A.append(_f64(0, LO, r)); B.append(_f64(0, HI, r[::-1]))           # down to 2^-513
    same = _f64(0, rng.integers(LO, HI + 1, size=1024, dtype=np.uint64), r[:1024])
    A.append(same); B.append(same)                                      # x / x
    spec = _specials()
    sa, sb = [x.ravel() for x in np.meshgrid(spec, spec)]
    A.append(sa); B.append(sb)                                          # excluded class / excluded class
    ordinary = _f64(0, rng.integers(LO, HI + 1, size=spec.size * 8, dtype=np.uint64),
                    rng.integers(0, 1 << 52, size=spec.size * 8, dtype=np.uint64))
    A.append(np.tile(spec, 8)); B.append(ordinary)                      # excluded / admitted
    A.append(ordinary); B.append(np.tile(spec, 8))                      # admitted / excluded
    out = _f64(0, rng.integers(1, 2047, size=4096, dtype=np.uint64), rng.integers(0, 1 << 52, size=4096, dtype=np.uint64))
    A.append(out); B.append(out[::-1])                                  # anywhere in the format: mostly refused
    a, b = np.concatenate(A), np.concatenate(B)
    assert a.size == b.size and a.size >= 60000
    return a, b


@pytest.fixture(scope="module")
def any_scene():
    ds = DeviceScene(gpu_launch.any_scene())
    yield ds
    ds.close()


@pytest.mark.parametrize("op,name", [(0, "sqrt"), (3, "sqrt and 1/sqrt"), (1, "1/x"), (2, "a/b")])
def test_guarded_primitives_are_bitwise_the_compilers(any_scene, op, name):
    rng = np.random.default_rng(20261020 + op)
    if op == 2:
        a, b = _quotient_operands(rng)
    else:
        a, b = _window_operands(rng, both_signs=op == 1), None
    hi = a.view(np.uint64) >> np.uint64(32)
    admitted = ((hi & np.uint64(0x7FFFFFFF if op in (1, 2) else 0xFFFFFFFF)) - np.uint64(LO << 20)) < np.uint64((HI - LO + 1) << 20)
    bad = any_scene.unscaled_check(op, a, b)
    print(f"{name}: {bad} of {a.size} operands differ ({int(np.count_nonzero(admitted))} with a in the window)")
    assert np.count_nonzero(admitted) > 30000 and np.count_nonzero(~admitted) > 3000
    assert bad == 0


def test_invalid_arguments_are_refused(any_scene):
    with pytest.raises(_abi.RaingunError):
        any_scene.unscaled_check(4, np.ones(4))
    with pytest.raises(_abi.RaingunError):
        any_scene.unscaled_check(2, np.ones(4))  # a / b without b


# ---------------------------------------------------------------- frames
WHITE = Color.from_str("#ffffff")
MIRROR = Material(Color.from_str("#ffd0a0"), 0.6, surface="Reflecting", reflectivity=0.5)


def _scaled(scene, k):
    """Every coordinate and radius times 2^k (an exact scaling; directions and normals stay)."""
    s = copy.deepcopy(scene)
    f = 2.0 ** k
    for b in s.bodies:
        if isinstance(b, Sphere):
            b.center = tuple(c * f for c in b.center)
            b.radius = b.radius * f
        else:
            assert isinstance(b, Plane)
            b.origin = tuple(c * f for c in b.origin)
    for l in s.lights:
        if isinstance(l, SphericalLight):
            l.position = tuple(c * f for c in l.position)
    return s


def _scenes(example_scenes):
    t1 = copy.deepcopy(example_scenes["test1"])
    t1.max_recursion_depth = 5
    floor = Material(Color.from_str("#c0c0c0"), 0.5)
    water = Material(Color.from_str("#f0fff0"), 0.2, surface="Refractive", index=1.33, transparency=0.9)
    anti = Material(Color.from_str("#fff0f0"), 0.2, surface="Refractive", index=1.0 / 1.33, transparency=0.9)
    up = float(np.nextafter(np.nextafter(np.nextafter(-2.0, 0.0), 0.0), 0.0))  # 3 ulps above the floor
    grid = [Sphere((-3.0 + 2.0 * i, -1.0 + 1.5 * j, -9.0 - 0.5 * ((i + j) % 3)), 0.15 + 0.04 * ((3 * i + j) % 5), MIRROR if (i + j) % 2 else floor)
            for i in range(4) for j in range(2)]
    return {
        "test1": t1,
        # coordinates ~2^-100: the squares under the spherical lights' square roots (the guarded
        # operands) are ~2^-200 -- inside the window [2^-256, 2^257) at every hit.
        "test1_2^-100": _scaled(t1, -100),
        # coordinates ~2^-300: those squares are ~2^-600, below the window, so every spherical light's
        # setup goes through the fallback in every lane, while every |coordinate| < 1e100 passes
        # ray_exotic.
        "test1_2^-300": _scaled(t1, -300),
        # a spherical light 3 ulps above the floor it lights: light distances (the setup's guarded
        # square root and reciprocal) down to ~1e-15 under it
        "light_on_plane": Scene(bodies=[Plane((0.0, -2.0, -5.0), (0.0, -1.0, 0.0), floor), Sphere((1.5, -1.0, -6.0), 1.0, MIRROR)],
                                lights=[SphericalLight((0.0, up, -6.0), Color.from_str("#ffffee"), 50.0),
                                        SphericalLight((-2.0, 3.0, -3.0), WHITE, 800.0)], max_recursion_depth=5),
        # 8 spheres a pixel or two across at 97x61: their hits graze (tiny r2 - opp in sphere_tail, which
        # stays the compiler's sqrt, as does the normal)
        "grazing": Scene(bodies=[Plane((0.0, -2.0, -5.0), (0.0, -1.0, 0.0), floor)] + grid,
                         lights=[SphericalLight((2.0, 3.0, -2.0), Color.from_str("#ffffee"), 700.0),
                                 DirectionalLight((0.3, -1.0, -0.4), WHITE, 1.5)], max_recursion_depth=5),
        # a refractive sphere around the camera (seen from inside, index 1.33) and beyond it one seen
        # from outside with index 1/1.33, over a floor
        "refract": Scene(bodies=[Plane((0.0, -2.5, -5.0), (0.0, -1.0, 0.0), floor), Sphere((0.2, 0.1, -1.0), 3.0, water),
                                 Sphere((0.8, -0.2, -8.0), 1.6, anti), Sphere((-2.5, 0.5, -9.0), 1.2, MIRROR)],
                         lights=[SphericalLight((2.0, 6.0, -4.0), Color.from_str("#ffffee"), 2500.0),
                                 DirectionalLight((0.3, -1.0, -0.4), WHITE, 1.5)],
                         default_color=Color.from_str("#203040"), max_recursion_depth=6),
        # the first directional light runs along x: the floor's denominator against it is 0, the wall's
        # at x = 6 is 1; the third runs 2e-6 off the floor's plane: a denominator just above the 1e-6
        # threshold.  (The planes' tests are the compiler's divisions; the scene guards the frames'
        # equality around the lights' setup.)
        "parallel": Scene(bodies=[Plane((0.0, -2.0, -5.0), (0.0, -1.0, 0.0), floor), Plane((6.0, 0.0, 0.0), (1.0, 0.0, 0.0), floor),
                                  Sphere((0.0, -0.5, -6.0), 1.2, MIRROR), Sphere((2.5, 0.0, -5.0), 0.8, floor)],
                          lights=[DirectionalLight((-1.0, 0.0, 0.0), WHITE, 2.0), SphericalLight((-2.0, 3.0, -3.0), WHITE, 600.0),
                                  DirectionalLight((0.0, 2e-6, -1.0), Color.from_str("#ffeedd"), 1.0)], max_recursion_depth=5),
    }


NAMES = ["test1", "test1_2^-100", "test1_2^-300", "light_on_plane", "grazing", "refract", "parallel"]


@pytest.mark.parametrize("mode", ["single", "pipelined"])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_frames(oracle_lib, example_scenes, name, w, h, mode):
    scene = _scenes(example_scenes)[name]
    o_rgba, o_counts = oracle_frame(oracle_lib, name, scene, w, h)
    ds = DeviceScene(scene)
    rgba, counts, plain, _ = device_launch(ds, w, h, mode)
    ds.set_exact_div(False)  # the same scene on the general kernel
    g_rgba, g_counts, g_plain, _ = device_launch(ds, w, h, mode)
    ds.close()
    assert plain and not g_plain, f"ran the {'PLAIN' if plain else 'general'} kernel, then the {'PLAIN' if g_plain else 'general'} one"
    assert counts == o_counts and g_counts == o_counts, "ray counts differ"
    mism = np.count_nonzero((rgba != o_rgba).any(axis=2))
    gmism = np.count_nonzero((rgba != g_rgba).any(axis=2))
    assert mism == 0 and gmism == 0, f"{mism} RGBA8 pixels differ from the CPU restatement, {gmism} from the general kernel"
