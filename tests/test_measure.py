"""scripts/rg_measure.py, the measuring loop the feature benchmarks share, on the CPU: the order in which
`alternate` runs its variants, `summary` by hand, the no-GPU exit, the nine scripts' option parsing, and the two
README writers against the committed records (which pins the readers of the record schema).
"""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
SCRIPTS = REPO / "scripts"
BENCHES = ["aa_bench", "aa_adaptive_bench", "camera_bench", "lens_bench", "area_bench", "aov_bench", "ao_bench",
           "ambient_bench", "pass_call_bench"]


@pytest.fixture(scope="module")
def rm():
    sys.path.insert(0, str(SCRIPTS))
    try:
        import rg_measure
    finally:
        sys.path.pop(0)
    return rg_measure


def _recorder():
    calls = []

    def batch_ms(fn):
        calls.append(fn())
        return float(len(calls))

    return calls, batch_ms


def test_alternate_order(rm):
    fns = {n: (lambda n=n: n) for n in "abc"}
    calls, batch_ms = _recorder()
    res = rm.alternate(fns, batch_ms, warmup=2, batches=3)
    assert calls == list("aabbcc") + list("abc") * 3
    # the counter's values, in call order: the warm-up batches are not among them
    assert res == {"a": [7.0, 10.0, 13.0], "b": [8.0, 11.0, 14.0], "c": [9.0, 12.0, 15.0]}
    assert list(res) == ["a", "b", "c"]


def test_alternate_without_warmup(rm):
    fns = {n: (lambda n=n: n) for n in "ab"}
    calls, batch_ms = _recorder()
    res = rm.alternate(fns, batch_ms, warmup=0, batches=2)
    assert calls == list("abab")
    assert res == {"a": [1.0, 3.0], "b": [2.0, 4.0]}


def test_summary(rm):
    assert rm.summary([3.0, 1.0, 2.5]) == {"median_ms": 2.5, "min_ms": 1.0, "max_ms": 3.0, "batches": 3}
    assert rm.summary([4.0, 1.0, 2.0, 3.0]) == {"median_ms": 2.5, "min_ms": 1.0, "max_ms": 4.0, "batches": 4}


def test_require_gpu(rm, monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit) as e:
        rm.require_gpu("some_bench.py")
    assert str(e.value) == "some_bench.py needs a GPU: nothing is measured without one"
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    rm.require_gpu("some_bench.py")


@pytest.mark.parametrize("script", BENCHES)
def test_help(script):
    p = subprocess.run([sys.executable, str(SCRIPTS / f"{script}.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "--batches" in p.stdout and "--warmup" in p.stdout and "--out" in p.stdout


@pytest.mark.parametrize("script,records", [("ao_bench", "ao"), ("ambient_bench", "ambient")])
def test_readme_from_the_committed_records(script, records, tmp_path):
    copy = tmp_path / records
    shutil.copytree(REPO / "profiles" / records, copy)
    committed = (copy / "README.md").read_bytes()
    (copy / "README.md").unlink()
    p = subprocess.run([sys.executable, str(SCRIPTS / f"{script}.py"), "--readme-only", "--dir", str(copy)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert (copy / "README.md").read_bytes() == committed


def test_the_loop_is_defined_once():
    """What `git grep -n "def batch_ms\\|def alternate\\|def _summary" scripts/` finds: rg_measure.py alone."""
    pat = re.compile(r"def batch_ms|def alternate|def _summary")
    found = sorted({f.name for f in SCRIPTS.iterdir() if f.is_file() and f.suffix in (".py", ".sh")
                    and pat.search(f.read_text())})
    assert found == ["rg_measure.py"]
