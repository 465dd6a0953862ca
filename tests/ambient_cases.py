"""The cases of the ambient term's tests, shared by tests/test_ambient_cpu.py (which checks the conditions on the
inputs, on the reference) and tests/test_gpu_ambient.py (which runs them on the GPU).

Scene cases: tests/ao_cases.py's scenes at 97x61, filtered with radius 2 and normal_min 0.9, two (k, radius, bias)
passes each with k >= 2.  A parity case proves little if the guides never stop the filter or the filter changes
nothing, so on the REFERENCE at least 5 % of the hit pixels must have an in-frame neighbour the filter rejects and
at least 50 % must change value.  The passes below were chosen on the CPU against that condition: k = 2 at +inf
where that meets it, and a second pass per scene; with a finite radius most of a small-k frame is exactly
1.0 and stays so (test1 k 2 radius 8: 41 % change; synth16 k 8 radius 32: 37 %), so the finite radii come with
k = 8 or not at all.  synth64, a closed room, is 0.0 everywhere at +inf; of its finite-radius passes (3, 24) and
(8, 16) meet the condition, (2, 16) does not (38 %); slab's k = 2 frame does not either (43 %).

Synthetic guide cases for the stand-alone filter (guides()): random f32 `ao` with full mantissas, body ids in
patches, non-unit normals jittered about a few directions, some NaN normals, some -1 bodies.  Conditions
(assert_guides): at radius 2 and normal_min 0.9 between 25 % and 75 % of the in-frame pairs are accepted, and
walking the taps backwards changes at least 40 % of the reference's outputs at every radius >= 2 -- so a reordered
sum cannot pass.
"""
import numpy as np

import ambient_ref
import ao_cases
from ao_cases import H, W

RADIUS, NORMAL_MIN = 2, 0.9
MIN_REJECTING, MIN_CHANGED = 0.05, 0.50
INF = float("inf")
CASES = {
    "test1": [(2, INF, 1e-13), (8, 8.0, 1e-6)],
    "test2": [(2, INF, 1e-13), (8, 8.0, 1e-6)],
    "test3": [(2, INF, 1e-13), (8, 8.0, 1e-6)],
    "open64": [(2, INF, 1e-13), (8, 24.0, 1e-6)],
    "synth16": [(2, INF, 1e-13), (3, INF, 1e-6)],
    "synth64": [(3, 24.0, 1e-6), (8, 16.0, 1e-13)],
    "slab": [(3, INF, 1e-6), (8, INF, 1e-13)],
}
SCENES = list(CASES)
# the stand-alone filter: sizes (w, h) and what they reach
SIZES = [(1, 1),      # the smallest frame
         (17, 3),     # the r = 8 window is larger than the frame
         (97, 61),    # several tiles both ways, partial tiles
         (261, 19),   # crosses a 256-column boundary
         (19, 261)]   # portrait
RADII = (1, 2, 3, 8)
NORMAL_MINS = (0.0, 0.9, 1.0)
ACCEPT_RANGE = (0.25, 0.75)
MIN_REORDERED = 0.40

_DIRECTIONS = np.array([(0, 0, 1), (0, 1, 0), (1, 0, 0), (0.6, 0.0, 0.8), (0, -1, 0), (-0.5, 0.5, 0.7)], np.float64)


def combos(name):
    """The scene's two (k, radius, bias) passes."""
    return CASES[name]


def guides(w, h, seed=0):
    """(ao (h, w) f32, body (h, w) i32, normal (h, w, 3) f32), read-only, the same arrays for the same arguments."""
    key = ("ambient guides", w, h, seed)

    def make():
        rng = np.random.default_rng([seed, w, h])
        # ao: sign 0, exponent 2^-6 .. 2^-1, every mantissa bit random
        bits = (rng.integers(121, 127, (h, w), dtype=np.uint32) << np.uint32(23)) | rng.integers(0, 1 << 23, (h, w), dtype=np.uint32)
        ao = bits.view(np.float32)
        # bodies and directions in patches of 24 x 16 pixels, the grid shifted so that frames start inside a patch
        py, px = (np.arange(h)[:, None] + 5) // 16, (np.arange(w)[None, :] + 7) // 24
        patch_body = rng.integers(0, 3, (py.max() + 1, px.max() + 1)).astype(np.int32)
        patch_dir = rng.integers(0, len(_DIRECTIONS), patch_body.shape)
        body = patch_body[py, px].copy()
        body[rng.random((h, w)) < 0.08] = -1
        n = _DIRECTIONS[patch_dir[py, px]] + rng.normal(0.0, 0.22, (h, w, 3))
        n *= rng.uniform(0.25, 4.0, (h, w, 1))  # not unit
        normal = n.astype(np.float32)
        bad = rng.random((h, w)) < 0.03
        normal[bad, rng.integers(0, 3, int(bad.sum()))] = np.nan
        return ao, body, normal

    import ref_lib

    return ref_lib.cached(key, make)


def assert_guides(w, h):
    """The conditions on the synthetic guides of a frame large enough to have windows (97x61 and up)."""
    ao, body, normal = guides(w, h)
    assert (body < 0).any() and np.isnan(normal).any() and (body >= 0).sum() > 0.8 * body.size
    n_pairs, n_accepted, _ = ambient_ref.pairs(body, normal, RADIUS, NORMAL_MIN)
    share = n_accepted / n_pairs
    assert ACCEPT_RANGE[0] <= share <= ACCEPT_RANGE[1], f"{w}x{h}: {share:.3f} of the in-frame pairs are accepted"
    for r in RADII:
        if r < 2:
            continue
        fwd = ambient_ref.filter_ao(ao, body, normal, r, NORMAL_MIN)
        rev = ambient_ref.filter_ao(ao, body, normal, r, NORMAL_MIN, reverse=True)
        changed = float((fwd.view(np.uint32) != rev.view(np.uint32)).mean())
        assert changed >= MIN_REORDERED, f"{w}x{h} r {r}: the reversed order changes only {changed:.3f} of the outputs"


def scene_layers(example_scenes, name, k, radius, bias, cam=None):
    """(raw ao, body, normal) of the scene's 97x61 frame on the reference."""
    import aov_ref

    scene = ao_cases.scene(example_scenes, name)
    st, layers, _, _ = aov_ref.cached(name, scene, W, H, cam)
    a_st, raw = ao_cases.ref(example_scenes, name, W, H, k, radius, bias, cam)[:2]
    assert st == 0 and a_st == 0, (name, st, a_st)
    return raw, layers["body"], layers["normal"]


def scene_shares(example_scenes, name, k, radius, bias):
    """(share of the hit pixels with a rejected in-frame neighbour, share of the hit pixels the filter changes)."""
    raw, body, normal = scene_layers(example_scenes, name, k, radius, bias)
    hit = body >= 0
    _, _, rejecting = ambient_ref.pairs(body, normal, RADIUS, NORMAL_MIN)
    out = ambient_ref.filter_ao(raw, body, normal, RADIUS, NORMAL_MIN)
    n = max(int(hit.sum()), 1)
    return float((rejecting & hit).sum()) / n, float(((out.view(np.uint32) != raw.view(np.uint32)) & hit).sum()) / n


def assert_condition(example_scenes, name):
    for k, radius, bias in combos(name):
        rejecting, changed = scene_shares(example_scenes, name, k, radius, bias)
        assert rejecting >= MIN_REJECTING, f"{name} k {k} radius {radius}: {rejecting:.3f} of the hit pixels reject a neighbour"
        assert changed >= MIN_CHANGED, f"{name} k {k} radius {radius}: the filter changes {changed:.3f} of the hit pixels"
