"""bench.py's run modes, on the CPU: a plain run measures the headline figure only (every other
measurement sits behind --full), and --dump-outputs writes the last step's loss / gradients / parameters /
normalizer statistics as float .npy files within its byte budget."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_measures_the_headline_only(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert a.cpu_steps == 0 and a.sustain == 0 and a.no_secondary and a.no_mse and a.no_profile
    # the selectors of the extra measurements do nothing without --full
    a = _parse(monkeypatch, "--cpu-steps", "5", "--sustain", "2")
    assert a.cpu_steps == 0 and a.sustain == 0


def test_full_run_keeps_every_measurement(monkeypatch):
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full and a.dump_outputs == "somewhere"
    assert a.cpu_steps == 10 and a.sustain == 5.0
    assert not (a.no_secondary or a.no_mse or a.no_profile)
    a = _parse(monkeypatch, "--full", "--cpu-steps", "0", "--no-mse")
    assert a.cpu_steps == 0 and a.no_mse and not a.no_profile


class _Sim(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(5, 3)
        self.b = torch.nn.Linear(3, 2, bias=False)
        self.register_buffer("count", torch.tensor(4.0))
        self.register_buffer("acc", torch.arange(6, dtype=torch.float32).reshape(1, 6))


def _stepped():
    torch.manual_seed(0)
    sim = _Sim()
    loss = sim.b(sim.a(torch.randn(7, 5))).square().mean()
    loss.backward()
    return sim, loss


def test_dump_outputs_writes_the_steps_arrays(tmp_path):
    sim, loss = _stepped()
    bench.dump_outputs(str(tmp_path / "out"), loss, sim)
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in sorted(os.listdir(tmp_path / "out"))}
    assert sorted(got) == ["grads", "loss", "normalizers", "params"]
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    ps = [p for _, p in sim.named_parameters()]
    np.testing.assert_array_equal(got["loss"], [loss.item()])
    np.testing.assert_array_equal(got["params"], torch.cat([p.detach().reshape(-1) for p in ps]).numpy())
    np.testing.assert_array_equal(got["grads"], torch.cat([p.grad.reshape(-1) for p in ps]).numpy())
    np.testing.assert_array_equal(got["normalizers"], [4.0, 0, 1, 2, 3, 4, 5])


def test_dump_outputs_samples_within_the_budget(tmp_path, monkeypatch):
    sim, loss = _stepped()
    n = sum(p.numel() for p in sim.parameters())  # 24 elements: 8 B each for params + grads
    budget = 4 + 56 + 5 * 128 + 16 * 10  # loss, normalizers, five .npy headers, 10 sampled elements
    monkeypatch.setattr(bench, "DUMP_BUDGET", budget)
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), loss, sim)
    one = {f[:-4]: np.load(tmp_path / "one" / f) for f in os.listdir(tmp_path / "one")}
    two = {f[:-4]: np.load(tmp_path / "two" / f) for f in os.listdir(tmp_path / "two")}
    assert sum(os.path.getsize(tmp_path / "one" / f) for f in os.listdir(tmp_path / "one")) <= budget
    idx = one["sample_index"].astype(np.int64)
    assert len(idx) == 10 and len(set(idx)) == 10 and (np.diff(idx) > 0).all() and idx.max() < n
    full = torch.cat([p.detach().reshape(-1) for _, p in sim.named_parameters()]).numpy()
    np.testing.assert_array_equal(one["params"], full[idx])
    assert sorted(one) == sorted(two) and all(np.array_equal(one[k], two[k]) for k in one)  # a fixed sample
