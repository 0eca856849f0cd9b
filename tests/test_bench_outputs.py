"""bench.py --dump-outputs: what the last timed step computed, as .npy files within the 64 MB budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """Arrays that fit are written whole in their own shape; one over its cap or over what is left of the total is
    written as the elements at fixed positions, the same ones on every call, and the total stays under the budget."""
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(20, 30, generator=g).bfloat16()
    met = torch.tensor([1.5, 0.25])
    params = torch.randn(5000, generator=g)
    arrays = [("logits", logits, np.float32, 700), ("metrics", met, np.float64, 1000),
              ("params", params, np.float32, 1000)]
    bench._dump_outputs(str(tmp_path / "a"), 0, arrays)
    a = _load(str(tmp_path / "a"))
    assert sorted(a) == ["logits.npy", "metrics.npy", "params.npy"]
    assert a["logits.npy"].dtype == np.float32 and a["logits.npy"].shape == (20, 30)
    assert np.array_equal(a["logits.npy"], logits.float().numpy())
    assert a["metrics.npy"].dtype == np.float64 and np.array_equal(a["metrics.npy"], [1.5, 0.25])
    assert a["params.npy"].dtype == np.float32 and a["params.npy"].shape == (1000 - 600 - 2,)
    assert np.isin(a["params.npy"], params.numpy()).all()
    assert sum(v.size for v in a.values()) <= 1000
    params2 = params.clone()
    params2[::2] += 1.0  # another build's values: same positions sampled, so the difference shows elementwise
    arrays[2] = ("params", params2, np.float32, 1000)
    bench._dump_outputs(str(tmp_path / "b"), 0, arrays)
    b = _load(str(tmp_path / "b"))
    d = b["params.npy"] - a["params.npy"]
    one = np.isclose(d, 1.0, atol=1e-5)
    assert ((d == 0.0) | one).all() and one.any() and (d == 0.0).any()
    bench._dump_outputs(str(tmp_path / "c"), 1, arrays[:2])
    assert sorted(os.listdir(tmp_path / "c")) == ["logits_rank1.npy", "metrics_rank1.npy"]


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(tmp_path):
    """One plain run: --steps is the number of timed steps, the result line has ms_per_step and leaves the --full
    fields null, and the dump holds the last step's logits / metrics and the updated parameters."""
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--batch-per-gpu", "8", "--image-size", "64",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", out], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["unit"] == "images/s" and rec["dtype"] == "bf16"
    assert abs(rec["value"] - 8 / (rec["ms_per_step"] * 1e-3)) <= 0.01 * rec["value"]
    assert rec["config"]["comm_selftest"] is None and rec["config"]["params_equal_across_ranks"] is None
    a = _load(out)
    assert sorted(a) == ["logits.npy", "metrics.npy", "params.npy"]
    assert a["logits.npy"].dtype == np.float32 and a["logits.npy"].shape == (8, 1000)
    assert a["metrics.npy"].dtype == np.float64 and a["params.npy"].dtype == np.float32
    assert a["params.npy"].ndim == 1 and a["params.npy"].size >= 11689512  # ResNet-18, whole (under the budget)
    assert all(np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 * 1000 * 1000
    assert abs(a["metrics.npy"][0] - rec["config"]["last_loss"]) <= 1e-4
    assert np.abs(a["logits.npy"]).max() > 0 and np.abs(a["params.npy"]).max() > 0
