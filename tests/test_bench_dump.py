"""bench.py --dump-outputs without a GPU: the sampling rules of benchkit/dump.py on CPU tensors, and the arguments bench.py refuses."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from benchkit.dump import _sample, dump_outputs   # noqa: E402

torch = pytest.importorskip("torch")


def words(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1 << 50, shape, generator=g, dtype=torch.int64)


def test_small_output_is_written_whole_and_exactly():
    t = words((4, 2, 3, 16), 1)
    arr, ent = _sample(torch, t, 1 << 20)
    assert ent["sample"] == "all" and arr.dtype == np.float64 and arr.shape == (4, 2, 3, 16)
    assert (arr.astype(np.int64) == t.numpy()).all()


def test_large_output_keeps_a_fixed_seeded_set_of_items():
    t = words((64, 2, 3, 16), 2)
    per_item = 2 * 3 * 16 * 8
    arr, ent = _sample(torch, t, 5 * per_item)
    assert ent["sample"] == "batch items" and len(ent["items"]) == 5 and arr.shape == (5, 2, 3, 16)
    assert (arr.astype(np.int64) == t.numpy()[ent["items"]]).all()
    assert _sample(torch, t, 5 * per_item)[1]["items"] == ent["items"]     # same items every run


def test_one_item_too_large_keeps_flat_positions():
    t = words((2, 1000), 3)
    arr, ent = _sample(torch, t, 80)
    assert ent["sample"] == "flat positions" and arr.shape == (10,) and ent["count"] == 10
    again, _ = _sample(torch, t, 80)
    assert (arr == again).all()


def test_word_beyond_float64_is_refused():
    t = words((2, 8), 4)
    t[1, 3] = 1 << 53
    with pytest.raises(ValueError):
        _sample(torch, t, 1 << 20)


def test_dump_writes_files_and_manifest_within_the_budget(tmp_path):
    wl = SimpleNamespace(outputs=lambda: {"ct_out": words((32, 2, 4, 64), 5)}, cfg={"workload": "test"})
    run = SimpleNamespace(torch=torch, world=1, rank=0, args=SimpleNamespace(steps=3, warmup=1))
    names = dump_outputs(run, wl, str(tmp_path), budget=8 * 2 * 4 * 64 * 8)
    assert names == ["ct_out.npy"]
    arr = np.load(tmp_path / "ct_out.npy")
    assert arr.shape == (8, 2, 4, 64) and arr.nbytes <= 8 * 2 * 4 * 64 * 8
    man = json.loads((tmp_path / "manifest.json").read_text())
    assert man["steps_plus_warmup"] == 4 and man["outputs"]["ct_out"]["shape"] == [32, 2, 4, 64]


@pytest.mark.parametrize("flags", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_refuses_nonsense_step_counts(flags):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + flags, capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and not [l for l in p.stdout.splitlines() if l.startswith("{")]
