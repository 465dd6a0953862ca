"""bench.py end to end on the GPU, at a small frame: a plain run times exactly
`--steps` frames and reports the headline line alone, `--dump-outputs` writes
the frame of the last timed step (byte for byte the frame the library's
one-launch render gives), and `--full` still adds what it moved."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BENCH = Path(__file__).resolve().parent.parent / "bench.py"
W, H = 320, 240
SMALL = ["--gpus", "1", "--width", str(W), "--height", str(H), "--settle-s", "0"]


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, str(BENCH), *SMALL, *args], capture_output=True, text=True, env=env,
                       timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_line_alone_and_dumps_its_last_frame(tmp_path, golden_dir):
    from raingun_amd.scene import DeviceScene, load_scene

    line = _bench("--steps", "11", "--warmup", "3", "--dump-outputs", str(tmp_path / "a"))
    assert line["steps"] == 11 and line["warmup"] == 3 and line["n_gpus"] == 1
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0
    rays = line["rays_per_frame"]["total"]
    # value is rays per frame over the time of one timed step; the line rounds ms_per_step to 1e-4 ms
    assert line["value"] == pytest.approx(rays / (line["ms_per_step"] * 1e-3) / 1e6,
                                          rel=0.5e-4 / line["ms_per_step"] + 1e-5)
    for moved in ("cpu_baseline", "kernel_ms", "host_visible", "test3_4k", "north_star_1024_spheres"):
        assert moved not in line
    assert sorted(f.name for f in (tmp_path / "a").iterdir()) == ["frame.npy"]
    a = np.load(tmp_path / "a" / "frame.npy")
    assert a.dtype == np.float32 and a.shape == (H, W, 4)

    scene = load_scene(golden_dir / "examples" / "test1.yml", texture_root=golden_dir)
    scene.max_recursion_depth = 5  # bench.py's test1 workload
    ds = DeviceScene(scene, device=0)
    ref = ds.render_image(W, H)
    ds.close()
    assert np.array_equal(a, ref.astype(np.float32))


def test_full_run_keeps_the_moved_figures():
    line = _bench("--full", "--steps", "5", "--warmup", "1", "--extra", "host_visible", "--extra-budget", "0.2")
    assert line["steps"] == 5 and line["kernel_ms"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["gpu_over_cpu"] > 0
    assert line["host_visible"]["pinned"]["ms_per_step"] > 0
