"""Supersampled anti-aliasing on the GPU (rg_render_image_aa, rg_render_aa_async,
rg_resolve_box) against the CPU restatement: the oracle renders the
samples*width x samples*height frame, whose rays are exactly the sub-pixel
samples (ray.rs:43-49), and raingun_amd.aa.resolve_box box-filters it in numpy.

The bar: RGBA8 byte-identical, f32 means within 1e-4 (end to end) or bit-identical
(the resolve kernel alone), per-class ray counts equal to the oracle's."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from gpu_launch import assert_same_pixels, native_cli_path, png, require_device
from raingun_amd import _abi, aa
from raingun_amd.color import Color
from raingun_amd.scene import AABB, DeviceScene, Material, Scene, SceneDesc
from raingun_amd.synth import synthetic_scene

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4  # the project's per-channel bound on pre-quantisation f32 RGB


@pytest.fixture(scope="module", autouse=True)
def _device():
    require_device()


# ---------------------------------------------------------------- 1. the resolve kernel alone
def _samples(w, h, k, seed):
    """Seeded samples in [-0.25, 1.25] with NaN, +-inf and exact n/255 values injected."""
    rng = np.random.default_rng(seed)
    rgb = rng.uniform(-0.25, 1.25, size=(k * h, k * w, 3)).astype(np.float32)
    flat = rgb.reshape(-1)
    specials = np.concatenate([np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0], np.float32),
                               (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)])
    n = max(1, flat.size // 16)
    flat[rng.integers(0, flat.size, size=n)] = specials[rng.integers(0, specials.size, size=n)]
    return rgb


def _gpu_resolve(rgb, k, want_rgb=True):
    h, w = rgb.shape[0] // k, rgb.shape[1] // k
    rgba = np.full((h, w, 4), 7, np.uint8)
    mean = np.full((h, w, 3), 7, np.float32) if want_rgb else None
    _abi.check(_abi.lib().rg_resolve_box(0, rgb.ctypes.data, w, h, k, rgba.ctypes.data,
                                         mean.ctypes.data if want_rgb else None), "rg_resolve_box")
    return mean, rgba


# (101, 75, 3): odd pitch, the dword path; (64, 40, 4): aligned; (1030, 2, 2): rows longer than a block's reach
RESOLVE_SHAPES = [(1, 1, 1), (5, 3, 2), (101, 75, 3), (64, 40, 4), (33, 17, 5), (24, 16, 8), (1030, 2, 2)]


@pytest.mark.parametrize("w,h,k", RESOLVE_SHAPES)
def test_resolve_kernel_matches_numpy_bit_for_bit(w, h, k):
    rgb = _samples(w, h, k, seed=1000 * k + w)
    want_mean, want_rgba = aa.resolve_box(rgb, k)
    mean, rgba = _gpu_resolve(rgb, k)
    assert np.array_equal(rgba, want_rgba), f"{np.count_nonzero((rgba != want_rgba).any(axis=2))} pixels differ"
    assert np.array_equal(mean.view(np.uint32), want_mean.view(np.uint32))
    _, rgba_only = _gpu_resolve(rgb, k, want_rgb=False)  # the f32 output is optional
    assert np.array_equal(rgba_only, want_rgba)


@pytest.mark.parametrize("w,h,k", [(12, 5, 1), (7, 4, 4), (20, 3, 6), (16, 9, 7)])
def test_resolve_kernel_other_alignments(w, h, k):
    """Widths whose sample pitch is 16-B aligned while the output rows are not (7 x 4), every
    remaining sample count, and k = 1."""
    rgb = _samples(w, h, k, seed=77 * k + w)
    want_mean, want_rgba = aa.resolve_box(rgb, k)
    mean, rgba = _gpu_resolve(rgb, k)
    assert np.array_equal(rgba, want_rgba)
    assert np.array_equal(mean.view(np.uint32), want_mean.view(np.uint32))


def test_device_scene_resolve_box(example_scenes):
    rgb = _samples(40, 24, 2, seed=5)
    ds = DeviceScene(example_scenes["test1"])
    mean, rgba = ds.resolve_box(rgb, 2)
    ds.close()
    want_mean, want_rgba = aa.resolve_box(rgb, 2)
    assert np.array_equal(rgba, want_rgba) and np.array_equal(mean.view(np.uint32), want_mean.view(np.uint32))


# ---------------------------------------------------------------- 2. end to end
_SCENES = {}
_EXPECTED = {}


def _scene(example_scenes, name):
    if name not in _SCENES:
        _SCENES[name] = synthetic_scene(64, 8, 8) if name == "synth64" else example_scenes[name]
    return _SCENES[name]


def _expected(oracle_lib, example_scenes, name, w, h, k):
    """The oracle at (k w, k h) resolved in numpy: computed once per scene and shape, read-only."""
    key = (name, w, h, k)
    if key not in _EXPECTED:
        st, _, rgb, counts, err = oracle_lib.render(SceneDesc(_scene(example_scenes, name)), k * w, k * h,
                                                    want_rgb=True)
        assert st == 0
        mean, rgba = aa.resolve_box(rgb, k)
        mean.setflags(write=False)
        rgba.setflags(write=False)
        _EXPECTED[key] = (mean, rgba, counts)
    return _EXPECTED[key]


@pytest.mark.parametrize("w,h,k", [(160, 90, 2), (101, 75, 3), (64, 40, 4)])
@pytest.mark.parametrize("path", [_abi.PATH_LIGHT, _abi.PATH_HEAVY])
@pytest.mark.parametrize("name", ["test1", "test2", "test3", "synth64"])
def test_supersampled_frame_matches_oracle(oracle_lib, example_scenes, name, path, w, h, k):
    want_mean, want_rgba, want_counts = _expected(oracle_lib, example_scenes, name, w, h, k)
    ds = DeviceScene(_scene(example_scenes, name), path=path)
    try:
        for band_rows in (0, 16, 7):  # automatic (one band at these sizes), several bands, a partial last band
            ds.set_aa_band_rows(band_rows)
            st = _abi.rg_stats()
            rgba, mean = ds.render_image_aa(w, h, k, want_rgb=True, stats=st)
            assert_same_pixels(rgba, want_rgba, f"band rows {band_rows}")
            diff = float(np.abs(mean.astype(np.float64) - want_mean.astype(np.float64)).max())
            assert diff <= RGB_TOL, f"band rows {band_rows}: f32 means differ by {diff}"
            assert st.rays.as_dict() == want_counts, f"band rows {band_rows}: ray counts differ"
            assert st.error_pixel == -1
            assert np.array_equal(ds.render_image_aa(w, h, k), want_rgba)  # without the f32 output
    finally:
        ds.close()


def test_pinned_destination(oracle_lib, example_scenes):
    """A registered (page-locked) caller buffer receives the bands' copies directly."""
    w, h, k = 160, 90, 2
    _, want_rgba, _ = _expected(oracle_lib, example_scenes, "test1", w, h, k)
    ds = DeviceScene(example_scenes["test1"])
    ds.set_aa_band_rows(16)
    out = np.zeros((h, w, 4), np.uint8)
    with _abi.HostRegistration(out):
        ds.render_image_aa(w, h, k, out=out)
    ds.close()
    assert np.array_equal(out, want_rgba)


# ---------------------------------------------------------------- 3. samples = 1
def test_one_sample_equals_render_image(example_scenes):
    ds = DeviceScene(example_scenes["test1"])
    whole = ds.render_image(160, 120)
    assert np.array_equal(ds.render_image_aa(160, 120, 1), whole)
    rgba, mean = ds.render_image_aa(160, 120, 1, want_rgb=True)  # through the resolve
    ds.close()
    assert np.array_equal(rgba, whole)
    assert np.array_equal(aa.f32_to_u8(mean * np.float32(255.0)), whole[..., :3])
    assert np.array_equal(example_scenes["test1"].render_image(160, 120, samples=1), whole)


def test_scene_render_image_samples_keyword(oracle_lib, example_scenes):
    _, want_rgba, _ = _expected(oracle_lib, example_scenes, "test1", 160, 90, 2)
    assert np.array_equal(example_scenes["test1"].render_image(160, 90, samples=2), want_rgba)


# ---------------------------------------------------------------- 4. device-resident
def test_async_equals_host_entry(example_scenes):
    import torch

    w, h, k = 160, 90, 2
    ds = DeviceScene(example_scenes["test3"])
    ds.set_aa_band_rows(16)
    st_host = _abi.rg_stats()
    want_rgba, want_mean = ds.render_image_aa(w, h, k, want_rgb=True, stats=st_host)
    lib = _abi.lib()
    stream = torch.cuda.Stream()
    rgba = torch.full((h, w, 4), 7, dtype=torch.uint8, device="cuda")
    mean = torch.full((h, w, 3), 7, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    # asynchronous (no stats), ordered on the caller's stream
    _abi.check(lib.rg_render_aa_async(ds.handle, w, h, k, C.c_void_p(rgba.data_ptr()), C.c_void_p(mean.data_ptr()),
                                      C.c_void_p(stream.cuda_stream), None), "rg_render_aa_async")
    with torch.cuda.stream(stream):
        got_rgba, got_mean = rgba.clone(), mean.clone()  # later work on the stream sees the frame
    stream.synchronize()
    assert np.array_equal(got_rgba.cpu().numpy(), want_rgba)
    assert np.array_equal(got_mean.cpu().numpy().view(np.uint32), want_mean.view(np.uint32))
    # with stats: synchronous, the host entry's counts; RGBA8 only
    rgba.fill_(7)
    torch.cuda.synchronize()
    st = _abi.rg_stats()
    _abi.check(lib.rg_render_aa_async(ds.handle, w, h, k, C.c_void_p(rgba.data_ptr()), None,
                                      C.c_void_p(stream.cuda_stream), C.byref(st)), "rg_render_aa_async")
    assert np.array_equal(rgba.cpu().numpy(), want_rgba)
    assert st.rays.as_dict() == st_host.rays.as_dict() and st.error_pixel == -1 and st.kernel_ms > 0
    ds.close()


# ---------------------------------------------------------------- 5. device errors
def test_device_error_names_the_output_pixel(oracle_lib):
    """tests/test_gpu_parity.py test_aabb_normal_error_matches_oracle's scene: the status is the
    oracle's at the sample frame's size, the pixel the output pixel holding the first failing sample."""
    m = Material(Color.from_str("#ffffff"), 0.5)
    s = Scene(bodies=[AABB(((-3e8, -3e8, -7e8), (3e8, 3e8, -5e8)), m)])
    w, h, k = 64, 48, 2
    o_st, _, o_rgb, _, o_err = oracle_lib.render(SceneDesc(s), k * w, k * h, want_rgb=True)
    assert o_st == _abi.RG_ERR_AABB_NORMAL and o_err >= 0
    want_pixel = (o_err // (k * w) // k) * w + (o_err % (k * w)) // k
    ds = DeviceScene(s)
    for band_rows in (0, 8):
        ds.set_aa_band_rows(band_rows)
        st = _abi.rg_stats()
        out = np.zeros((h, w, 4), np.uint8)
        status = _abi.lib().rg_render_image_aa(ds.handle, w, h, k, out.ctypes.data, None, C.byref(st))
        assert status == o_st
        assert st.error_pixel == want_pixel
        assert (out[..., 3] == 255).all()  # the frame is still delivered
    with pytest.raises(_abi.RaingunError) as ei:
        ds.render_image_aa(w, h, k)
    assert ei.value.status == o_st
    ds.close()


# ---------------------------------------------------------------- 6. argument errors
def test_argument_errors(example_scenes):
    ds = DeviceScene(example_scenes["test2"])
    with pytest.raises(_abi.RaingunError) as ei:
        ds.render_image_aa(60, 80, 2)
    assert ei.value.status == _abi.RG_ERR_PORTRAIT
    out = np.zeros((8, 8, 4), np.uint8)
    lib = _abi.lib()
    for k in (0, 9):
        assert lib.rg_render_image_aa(ds.handle, 8, 8, k, out.ctypes.data, None, None) == _abi.RG_ERR_INVALID_ARGUMENT
        assert lib.rg_render_aa_async(ds.handle, 8, 8, k, out.ctypes.data, None, None,
                                      None) == _abi.RG_ERR_INVALID_ARGUMENT
    assert lib.rg_render_image_aa(ds.handle, 8, 8, 2, None, None, None) == _abi.RG_ERR_INVALID_ARGUMENT
    assert lib.rg_render_image_aa(ds.handle, 0, 8, 2, out.ctypes.data, None, None) == _abi.RG_ERR_INVALID_ARGUMENT
    assert lib.rg_render_image_aa(ds.handle, 1 << 15, 1 << 15, 2, out.ctypes.data, None,
                                  None) == _abi.RG_ERR_INVALID_ARGUMENT  # 2^32 samples
    assert lib.rg_debug_set_aa_band_rows(ds.handle, -1) == _abi.RG_ERR_INVALID_ARGUMENT
    ds.close()


# ---------------------------------------------------------------- 7. command lines
@pytest.fixture(scope="module")
def native_cli():
    return native_cli_path()


def test_native_cli_samples(native_cli, oracle_lib, example_scenes, golden_dir, tmp_path):
    _, want_rgba, _ = _expected(oracle_lib, example_scenes, "test1", 160, 90, 2)
    out = tmp_path / "aa.png"
    yml = str(golden_dir / "examples" / "test1.yml")
    r = subprocess.run([native_cli, "--samples", "2", "-w", "160", "-h", "90", yml, "-o", str(out)],
                       cwd=golden_dir, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(png(out), want_rgba)
    r = subprocess.run([native_cli, "--samples", "x", yml, "-o", str(out)], cwd=golden_dir, capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 101 and "Could not parse samples" in r.stderr
    for v in ("0", "9"):
        r = subprocess.run([native_cli, "--samples", v, yml, "-o", str(out)], cwd=golden_dir, capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 1 and "--samples" in r.stderr
    r = subprocess.run([native_cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--samples" in r.stdout


def test_python_cli_samples(oracle_lib, example_scenes, golden_dir, tmp_path, monkeypatch):
    from raingun_amd.cli import main

    _, want_rgba, _ = _expected(oracle_lib, example_scenes, "test1", 160, 90, 2)
    out = tmp_path / "aa.png"
    monkeypatch.chdir(golden_dir)  # textures resolve against the working directory
    assert main(["--samples", "2", "-w", "160", "-h", "90", str(golden_dir / "examples" / "test1.yml"),
                 "-o", str(out)]) == 0
    assert np.array_equal(png(out), want_rgba)
