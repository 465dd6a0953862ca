"""Adaptive anti-aliasing on the GPU (rg_render_image_aa_adaptive, rg_render_aa_adaptive,
rg_edge_mask) against the CPU restatement: the oracle renders the 1-sample frame at W x H and
the sample frame at k W x k H, and raingun_amd.aa.resolve_adaptive combines them in numpy.

The bar: RGBA8 and mask byte-identical, f32 means within 1e-4, primary rays exactly
W H + k k F with F the flagged pixels of the oracle's own 1-sample frame."""
import ctypes as C

import numpy as np
import pytest

from gpu_launch import assert_same_pixels, require_device
from raingun_amd import _abi, aa
from raingun_amd.color import Color
from raingun_amd.scene import AABB, DeviceScene, Material, Scene, SceneDesc
from raingun_amd.synth import synthetic_scene

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4  # the project's per-channel bound on pre-quantisation f32 RGB


@pytest.fixture(scope="module", autouse=True)
def _device():
    require_device()


# ---------------------------------------------------------------- 1. the mask kernel alone
def _planted(w, h, t, seed):
    """Seeded random RGBA8 with planted runs whose neighbours differ by exactly +-t and by t -+ 1."""
    rng = np.random.default_rng(seed)
    rgba = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    # flat patches, so that thresholds below 255 leave something unflagged
    for _ in range(max(1, (w * h) // 64)):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        rgba[y:y + 6, x:x + 24, :3] = rng.integers(0, 256, size=3, dtype=np.uint8)
    d = min(max(t, 1), 255)
    for _ in range(max(1, (w * h) // 32)):  # runs of exact differences inside flat stretches
        y, x, c = int(rng.integers(0, h)), int(rng.integers(0, w)), int(rng.integers(0, 3))
        base = int(rng.integers(0, 256 - d))
        delta = d + int(rng.integers(-1, 2))  # t - 1, t, t + 1
        run = np.full((3,), base, np.int32)
        rgba[max(0, y - 1):y + 2, x:x + 8, :3] = base
        run[c] = min(255, base + delta) if rng.integers(0, 2) else base
        rgba[y, x + 3:x + 5, :3] = run.astype(np.uint8)
    return rgba


MASK_SHAPES = [(1, 1), (2, 1), (5, 3), (101, 75), (64, 40), (257, 9), (1030, 2)]  # (1030, 2): rows longer than a block's reach


@pytest.mark.parametrize("t", [0, 1, 32, 255, 256])
@pytest.mark.parametrize("w,h", MASK_SHAPES)
def test_mask_kernel_matches_numpy(w, h, t):
    rgba = _planted(w, h, t, seed=1000 * t + w)
    want = aa.edge_mask(rgba, t)
    mask = np.full((h, w), 7, np.uint8)
    n = C.c_uint32(0xFFFFFFFF)
    _abi.check(_abi.lib().rg_edge_mask(0, rgba.ctypes.data, w, h, t, mask.ctypes.data, C.byref(n)), "rg_edge_mask")
    assert np.array_equal(mask, want), f"{np.count_nonzero(mask != want)} mask bytes differ"
    assert n.value == int(want.sum())
    if w * h > 64 and 1 <= t <= 255:
        assert 0 < want.sum() < want.size  # the inputs exercise both outcomes


def test_mask_kernel_unaligned_and_optional_count(example_scenes):
    """A width that is a multiple of 4 (the 16-B path), one that is not, and no count."""
    for w, h in ((64, 5), (66, 5)):
        rgba = _planted(w, h, 32, seed=w)
        mask = np.empty((h, w), np.uint8)
        _abi.check(_abi.lib().rg_edge_mask(0, rgba.ctypes.data, w, h, 32, mask.ctypes.data, None), "rg_edge_mask")
        assert np.array_equal(mask, aa.edge_mask(rgba, 32))
    ds = DeviceScene(example_scenes["test1"])
    rgba = _planted(40, 24, 16, seed=4)
    mask, n = ds.edge_mask(rgba, 16)
    ds.close()
    assert np.array_equal(mask, aa.edge_mask(rgba, 16)) and n == int(mask.sum())


# ---------------------------------------------------------------- 2. end to end
_SCENES = {}
_ORACLE = {}


def _scene(example_scenes, name):
    if name not in _SCENES:
        _SCENES[name] = synthetic_scene(64, 8, 8) if name == "synth64" else example_scenes[name]
    return _SCENES[name]


def _oracle(oracle_lib, example_scenes, name, w, h):
    """The oracle's frame of a scene at one size: computed once, read-only."""
    key = (name, w, h)
    if key not in _ORACLE:
        st, rgba, rgb, counts, err = oracle_lib.render(SceneDesc(_scene(example_scenes, name)), w, h, want_rgb=True)
        assert st == 0
        rgba.setflags(write=False)
        rgb.setflags(write=False)
        _ORACLE[key] = (rgba, rgb, counts)
    return _ORACLE[key]


def _expected(oracle_lib, example_scenes, name, w, h, k, t):
    base_rgba, base_rgb, base_counts = _oracle(oracle_lib, example_scenes, name, w, h)
    _, s_rgb, s_counts = _oracle(oracle_lib, example_scenes, name, k * w, k * h)
    mean, rgba, mask = aa.resolve_adaptive(base_rgba, base_rgb, s_rgb, k, t)
    return mean, rgba, mask, base_counts, s_counts


@pytest.mark.parametrize("w,h,k", [(160, 90, 2), (101, 75, 3), (64, 40, 4)])
@pytest.mark.parametrize("path", [_abi.PATH_LIGHT, _abi.PATH_HEAVY])
@pytest.mark.parametrize("name", ["test1", "test2", "test3", "synth64"])
def test_adaptive_frame_matches_oracle(oracle_lib, example_scenes, name, path, w, h, k):
    t = 32
    want_mean, want_rgba, want_mask, base_counts, full_counts = _expected(oracle_lib, example_scenes, name, w, h, k, t)
    flagged = int(want_mask.sum())
    share = flagged / (w * h)
    print(f"{name} {w}x{h} k={k}: flagged share {share:.3f}")
    assert 0.03 <= share <= 0.70, f"the case is vacuous: flagged share {share:.3f}"
    ds = DeviceScene(_scene(example_scenes, name), path=path)
    try:
        for band_rows in (0, 16, 7):  # automatic (one band), several bands, bands that split sample tiles and pixels
            ds.set_aa_band_rows(band_rows)
            st = _abi.rg_stats()
            rgba, mean, mask = ds.render_image_aa_adaptive(w, h, k, t, want_rgb=True, want_mask=True, stats=st)
            assert np.array_equal(mask, want_mask), f"band rows {band_rows}: {np.count_nonzero(mask != want_mask)} mask bytes differ"
            assert_same_pixels(rgba, want_rgba, f"band rows {band_rows}")
            diff = float(np.abs(mean.astype(np.float64) - want_mean.astype(np.float64)).max())
            assert diff <= RGB_TOL, f"band rows {band_rows}: f32 means differ by {diff}"
            rays = st.rays.as_dict()
            print(f"  band rows {band_rows}: rays {rays}, base {base_counts}, full {full_counts}")
            assert rays["primary"] == w * h + k * k * flagged, f"band rows {band_rows}: primary rays"
            for cls in ("shadow", "secondary"):
                assert base_counts[cls] <= rays[cls] <= base_counts[cls] + full_counts[cls], f"band rows {band_rows}: {cls}"
            assert st.error_pixel == -1
            assert np.array_equal(ds.render_image_aa_adaptive(w, h, k, t), want_rgba)  # RGBA8 alone
    finally:
        ds.close()


# ---------------------------------------------------------------- 3. the limits of T, and k = 1
@pytest.mark.parametrize("name", ["test1", "synth64"])
def test_threshold_limits_and_one_sample(oracle_lib, example_scenes, name):
    w, h, k = 101, 75, 3
    base_rgba, base_rgb, base_counts = _oracle(oracle_lib, example_scenes, name, w, h)
    _, s_rgb, full_counts = _oracle(oracle_lib, example_scenes, name, k * w, k * h)
    box_mean, box_rgba = aa.resolve_box(s_rgb, k)
    ds = DeviceScene(_scene(example_scenes, name))
    try:
        ds.set_aa_band_rows(16)
        # T = 0: rg_render_image_aa, no base pass
        st = _abi.rg_stats()
        rgba, mean, mask = ds.render_image_aa_adaptive(w, h, k, 0, want_rgb=True, want_mask=True, stats=st)
        assert np.array_equal(rgba, box_rgba) and (mask == 1).all()
        assert float(np.abs(mean.astype(np.float64) - box_mean.astype(np.float64)).max()) <= RGB_TOL
        assert st.rays.as_dict() == full_counts and st.error_pixel == -1
        # T = 256: the 1-sample frame, nothing flagged
        st = _abi.rg_stats()
        rgba, mean, mask = ds.render_image_aa_adaptive(w, h, k, 256, want_rgb=True, want_mask=True, stats=st)
        assert np.array_equal(rgba, base_rgba) and (mask == 0).all()
        assert float(np.abs(mean.astype(np.float64) - aa.clamp_sample(base_rgb).astype(np.float64)).max()) <= RGB_TOL
        assert st.rays.as_dict() == base_counts and st.error_pixel == -1
        # k = 1 at T = 32: the 1-sample frame, with the mask of the definition
        want_mask = aa.edge_mask(base_rgba, 32)
        for want_rgb in (False, True):
            st = _abi.rg_stats()
            res = ds.render_image_aa_adaptive(w, h, 1, 32, want_rgb=want_rgb, want_mask=True, stats=st)
            assert np.array_equal(res[0], base_rgba) and np.array_equal(res[-1], want_mask)
            assert st.rays.as_dict() == base_counts and st.error_pixel == -1
            if want_rgb:
                assert float(np.abs(res[1].astype(np.float64) - aa.clamp_sample(base_rgb).astype(np.float64)).max()) <= RGB_TOL
        st = _abi.rg_stats()
        assert np.array_equal(ds.render_image_aa_adaptive(w, h, 1, 32, stats=st), base_rgba)
        assert st.rays.as_dict() == base_counts
    finally:
        ds.close()


def test_scene_render_image_adaptive_keyword(oracle_lib, example_scenes):
    _, want_rgba, _, _, _ = _expected(oracle_lib, example_scenes, "test1", 160, 90, 2, 32)
    assert np.array_equal(example_scenes["test1"].render_image(160, 90, samples=2, adaptive=32), want_rgba)


# ---------------------------------------------------------------- 4. device-resident
@pytest.mark.parametrize("name,path", [("test3", _abi.PATH_LIGHT), ("synth64", _abi.PATH_HEAVY)])
def test_device_entry_equals_host_entry(example_scenes, name, path):
    import torch

    w, h, k, t = 160, 90, 2, 32
    ds = DeviceScene(_scene(example_scenes, name), path=path)
    ds.set_aa_band_rows(16)
    st_host = _abi.rg_stats()
    want_rgba, want_mean, want_mask = ds.render_image_aa_adaptive(w, h, k, t, want_rgb=True, want_mask=True,
                                                                  stats=st_host)
    lib = _abi.lib()
    stream = torch.cuda.Stream()
    rgba = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    mean = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    big = torch.zeros((64 << 20,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = _abi.rg_stats()
    with torch.cuda.stream(stream):
        for _ in range(8):
            big.add_(1)  # work in front of the call on the caller's stream ...
        rgba.fill_(7)    # ... ending in a store the frame must come after
        mean.fill_(7)
        mask.fill_(7)
    _abi.check(lib.rg_render_aa_adaptive(ds.handle, w, h, k, t, C.c_void_p(rgba.data_ptr()), C.c_void_p(mean.data_ptr()),
                                         C.c_void_p(mask.data_ptr()), C.c_void_p(stream.cuda_stream), C.byref(st)),
               "rg_render_aa_adaptive")
    with torch.cuda.stream(stream):
        got_rgba, got_mean, got_mask = rgba.clone(), mean.clone(), mask.clone()  # later work on the stream sees the frame
        rgba.fill_(9)
    stream.synchronize()
    assert np.array_equal(got_rgba.cpu().numpy(), want_rgba)
    assert np.array_equal(got_mean.cpu().numpy().view(np.uint32), want_mean.view(np.uint32))
    assert np.array_equal(got_mask.cpu().numpy(), want_mask)
    assert (rgba.cpu().numpy() == 9).all()
    assert st.rays.as_dict() == st_host.rays.as_dict() and st.error_pixel == -1 and st.kernel_ms > 0
    # RGBA8 alone, no stats, the null stream; then T = 0 and k = 1 through the same entry
    rgba.fill_(7)
    torch.cuda.synchronize()
    _abi.check(lib.rg_render_aa_adaptive(ds.handle, w, h, k, t, C.c_void_p(rgba.data_ptr()), None, None, None, None),
               "rg_render_aa_adaptive")
    assert np.array_equal(rgba.cpu().numpy(), want_rgba)
    _abi.check(lib.rg_render_aa_adaptive(ds.handle, w, h, k, 0, C.c_void_p(rgba.data_ptr()), None,
                                         C.c_void_p(mask.data_ptr()), C.c_void_p(stream.cuda_stream), None))
    assert np.array_equal(rgba.cpu().numpy(), ds.render_image_aa(w, h, k)) and (mask.cpu().numpy() == 1).all()
    _abi.check(lib.rg_render_aa_adaptive(ds.handle, w, h, 1, t, C.c_void_p(rgba.data_ptr()), None, None,
                                         C.c_void_p(stream.cuda_stream), None))
    assert np.array_equal(rgba.cpu().numpy(), ds.render_image(w, h))
    ds.close()


# ---------------------------------------------------------------- 5. device errors
def test_device_error(oracle_lib):
    """tests/test_gpu_host_paths.py's AABB-normal scene: the oracle's status, the frame delivered, and the
    error pixel of the definition."""
    m = Material(Color.from_str("#ffffff"), 0.5)
    s = Scene(bodies=[AABB(((-3e8, -3e8, -7e8), (3e8, 3e8, -5e8)), m)])
    w, h, k = 64, 48, 2
    b_st, b_rgba, _, _, b_err = oracle_lib.render(SceneDesc(s), w, h, want_rgb=True)
    s_st, _, _, _, s_err = oracle_lib.render(SceneDesc(s), k * w, k * h, want_rgb=True)
    assert b_st == s_st == _abi.RG_ERR_AABB_NORMAL and b_err >= 0 and s_err >= 0
    s_pixel = (s_err // (k * w) // k) * w + (s_err % (k * w)) // k  # the output pixel of the first failing sample
    ds = DeviceScene(s)
    for band_rows in (0, 8):
        ds.set_aa_band_rows(band_rows)
        for t in (0, 32):
            st = _abi.rg_stats()
            out = np.zeros((h, w, 4), np.uint8)
            mask = np.zeros((h, w), np.uint8)
            status = _abi.lib().rg_render_image_aa_adaptive(ds.handle, w, h, k, t, out.ctypes.data, None,
                                                            mask.ctypes.data, C.byref(st))
            assert status == b_st
            assert (out[..., 3] == 255).all()  # the frame is still delivered
            if t == 0:  # no base pass: the sample frame's pixel
                assert st.error_pixel == s_pixel
            else:
                assert np.array_equal(mask, aa.edge_mask(b_rgba, t))
                assert 0 <= st.error_pixel <= b_err  # the lower of the two
                if mask.reshape(-1)[s_pixel]:        # the first failing sample was traced
                    assert st.error_pixel == min(b_err, s_pixel)
                if not mask.any():
                    assert st.error_pixel == b_err
    with pytest.raises(_abi.RaingunError) as ei:
        ds.render_image_aa_adaptive(w, h, k, 32)
    assert ei.value.status == b_st
    ds.close()


# ---------------------------------------------------------------- 6. argument errors
def test_argument_errors(example_scenes):
    ds = DeviceScene(example_scenes["test2"])
    lib = _abi.lib()
    out = np.full((8, 8, 4), 7, np.uint8)
    rgb = np.full((8, 8, 3), 7, np.float32)
    mask = np.full((8, 8), 7, np.uint8)
    o, r, m = out.ctypes.data, rgb.ctypes.data, mask.ctypes.data
    bad = _abi.RG_ERR_INVALID_ARGUMENT
    for entry, tail in ((lib.rg_render_image_aa_adaptive, (None,)), (lib.rg_render_aa_adaptive, (None, None))):
        assert entry(None, 8, 8, 2, 32, o, r, m, *tail) == bad
        assert entry(ds.handle, 8, 8, 2, 32, None, r, m, *tail) == bad
        assert entry(ds.handle, 0, 8, 2, 32, o, r, m, *tail) == bad
        assert entry(ds.handle, 8, 0, 2, 32, o, r, m, *tail) == bad
        assert entry(ds.handle, 8, 8, 0, 32, o, r, m, *tail) == bad
        assert entry(ds.handle, 8, 8, 9, 32, o, r, m, *tail) == bad
        assert entry(ds.handle, 8, 8, 2, 257, o, r, m, *tail) == bad
        assert entry(ds.handle, 1 << 15, 1 << 15, 2, 32, o, r, m, *tail) == bad  # 2^32 samples
        assert entry(ds.handle, 6, 8, 2, 32, o, r, m, *tail) == _abi.RG_ERR_PORTRAIT
    n = C.c_uint32(7)
    assert lib.rg_edge_mask(0, None, 8, 8, 32, m, C.byref(n)) == bad
    assert lib.rg_edge_mask(0, o, 8, 8, 32, None, C.byref(n)) == bad
    assert lib.rg_edge_mask(0, o, 0, 8, 32, m, C.byref(n)) == bad
    assert lib.rg_edge_mask(0, o, 8, 0, 32, m, C.byref(n)) == bad
    assert lib.rg_edge_mask(0, o, 8, 8, 257, m, C.byref(n)) == bad
    assert lib.rg_edge_mask(-1, o, 8, 8, 32, m, C.byref(n)) == bad
    assert (out == 7).all() and (rgb == 7).all() and (mask == 7).all() and n.value == 7  # nothing was touched
    with pytest.raises(_abi.RaingunError) as ei:
        ds.render_image_aa_adaptive(60, 80, 2, 32)
    assert ei.value.status == _abi.RG_ERR_PORTRAIT
    ds.close()


# ---------------------------------------------------------------- 7. repeated calls
def test_repeated_calls_with_changing_shapes(oracle_lib, example_scenes):
    """One scene, (k, T, size) changing from call to call: the slots, lists and mask buffers grow and are
    reused; a full supersampled frame in between uses the same streams and slots."""
    ds = DeviceScene(_scene(example_scenes, "test1"))
    try:
        ds.set_aa_band_rows(16)
        for w, h, k, t in [(64, 40, 4, 32), (160, 90, 2, 32), (64, 40, 4, 32), (101, 75, 3, 32), (160, 90, 2, 32)]:
            want_mean, want_rgba, want_mask, _, _ = _expected(oracle_lib, example_scenes, "test1", w, h, k, t)
            st = _abi.rg_stats()
            rgba, mask = ds.render_image_aa_adaptive(w, h, k, t, want_mask=True, stats=st)
            assert np.array_equal(rgba, want_rgba) and np.array_equal(mask, want_mask)
            assert st.rays.primary == w * h + k * k * int(want_mask.sum())
            if (w, h, k) == (101, 75, 3):
                _, s_rgb, _ = _oracle(oracle_lib, example_scenes, "test1", k * w, k * h)
                assert np.array_equal(ds.render_image_aa(w, h, k), aa.resolve_box(s_rgb, k)[1])
        # other thresholds on one size: the mask changes, the buffers stay
        w, h, k = 160, 90, 2
        for t in (1, 128, 255):
            _, want_rgba, want_mask, _, _ = _expected(oracle_lib, example_scenes, "test1", w, h, k, t)
            rgba, mask = ds.render_image_aa_adaptive(w, h, k, t, want_mask=True)
            assert np.array_equal(rgba, want_rgba) and np.array_equal(mask, want_mask)
    finally:
        ds.close()
