"""scripts/rg_measure.py on the GPU: the event-timed batch and the alternation around a real launch on a side
stream, and `Launches.frame` against the hand-written launch of tests/gpu_launch.py (test1 at 97x61: partial
tiles at the right and bottom edges).
"""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

from gpu_launch import device_launch, require_device
from raingun_amd.scene import DeviceScene

pytestmark = pytest.mark.gpu

SCRIPTS = Path(__file__).resolve().parents[1] / "scripts"
W, H = 97, 61


@pytest.fixture(scope="module", autouse=True)
def _device():
    require_device()


def test_alternate_times_a_launch_and_leaves_its_frame(example_scenes):
    import torch

    sys.path.insert(0, str(SCRIPTS))
    try:
        import rg_measure as rm
    finally:
        sys.path.pop(0)
    ds = DeviceScene(example_scenes["test1"])
    try:
        stream = torch.cuda.Stream()
        rgba = torch.full((H, W, 4), 7, dtype=torch.uint8, device="cuda")
        other = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        la = rm.Launches(ds, W, H, stream)
        with torch.cuda.stream(stream):
            r = rm.alternate({"frame": lambda: la.frame(rgba), "fill": lambda: other.fill_(1)},
                             rm.event_batch_ms(stream, 2), warmup=1, batches=2)
        assert list(r) == ["frame", "fill"]
        for ms in r.values():
            assert len(ms) == 2 and all(math.isfinite(v) and v > 0 for v in ms), r
        assert ds.stream_status(stream.cuda_stream) == (0, -1)
        stream.synchronize()
        got = rgba.cpu().numpy()
        ds.release_stream(stream.cuda_stream)
        assert np.array_equal(got, device_launch(ds, W, H).rgba)
    finally:
        ds.close()
