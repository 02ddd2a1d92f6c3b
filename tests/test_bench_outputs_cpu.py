"""bench.py --dump-outputs and --steps, on CPU: the dump holds float32 arrays of a fixed sample of the parameters and their
gradients (the same positions whatever the flat buffer's layout), and a run that would time no step is refused."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from multimeditron_amd.nn import FlatParams  # noqa: E402


class _Trainer:
    def __init__(self, named):
        self.flat = FlatParams([(n, p, "llm") for n, p in named], torch.device("cpu"), torch.float32)
        self.flat.ensure_grad()
        for seg in self.flat.segments:
            self.flat.grad[seg.start:seg.end] = -self.flat.data[seg.start:seg.end]

    def synchronize(self):
        pass


def _named(order):
    g = torch.Generator().manual_seed(0)
    shapes = {"a.weight": (300, 70), "b.weight": (5,), "c.bias": (9000,)}
    ps = {n: torch.nn.Parameter(torch.randn(*s, generator=g)) for n, s in shapes.items()}
    return [(n, ps[n]) for n in order]


def test_dump_outputs_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    loss = torch.tensor(2.5)
    bench.dump_outputs(str(tmp_path / "x"), _Trainer(_named(["a.weight", "b.weight", "c.bias"])), loss)
    bench.dump_outputs(str(tmp_path / "y"), _Trainer(_named(["c.bias", "b.weight", "a.weight"])), loss)
    for name in ("loss", "params", "grads"):
        x, y = np.load(tmp_path / "x" / f"{name}.npy"), np.load(tmp_path / "y" / f"{name}.npy")
        assert x.dtype == np.float32 and x.shape == y.shape
        np.testing.assert_array_equal(x, y)
    p, gr = np.load(tmp_path / "x" / "params.npy"), np.load(tmp_path / "x" / "grads.npy")
    assert p.shape == (4096 + 5 + 4096,)
    np.testing.assert_array_equal(gr, -p)
    assert np.load(tmp_path / "x" / "loss.npy").tolist() == [2.5]
    # a small tensor is dumped whole, in order
    np.testing.assert_array_equal(p[4096:4096 + 5], _named(["b.weight"])[0][1].detach().numpy())


def test_dump_outputs_size_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    named = [(f"p{i:03d}", torch.nn.Parameter(torch.zeros(5000))) for i in range(100)]
    bench.dump_outputs(str(tmp_path), _Trainer(named), torch.tensor(0.0), max_elems=20_000)
    assert np.load(tmp_path / "params.npy").size + np.load(tmp_path / "grads.npy").size <= 20_000


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--dry-run"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps" in r.stderr
