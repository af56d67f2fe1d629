"""bench.py's command line and --dump-outputs writer.  CPU only (no engine call)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_not_full(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.dump_outputs, a.steps, a.warmup, a.workload) == (False, None, 7, 2, "c2")
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"


def test_dump_sample_is_fixed_and_bounded():
    t = torch.arange(3 * bench.DUMP_SAMPLE, dtype=torch.int32)
    s1, s2 = bench.dump_sample(t), bench.dump_sample(t.clone())
    assert s1.numel() == bench.DUMP_SAMPLE and torch.equal(s1, s2)
    assert torch.all(s1[1:] > s1[:-1])  # distinct positions, in order
    small = torch.arange(10)
    assert bench.dump_sample(small) is small


def test_dump_outputs_writes_float64_npy(tmp_path):
    d = tmp_path / "out"
    bench.dump_outputs(str(d), 0, {"count": torch.tensor([50_000_017]),
                                   "flags": torch.tensor([0, 1, 1], dtype=torch.uint8)})
    bench.dump_outputs(str(d), 1, {"count": np.array([3], np.uint64)})
    assert sorted(os.listdir(d)) == ["count.npy", "count_rank1.npy", "flags.npy"]
    c, f = np.load(d / "count.npy"), np.load(d / "flags.npy")
    assert c.dtype == np.float64 and c.tolist() == [50_000_017.0]
    assert f.dtype == np.float64 and f.tolist() == [0.0, 1.0, 1.0]
