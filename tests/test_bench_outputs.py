"""bench.py's plain / --full switch and --dump-outputs (host logic only: the arrays are
CPU tensors behind a stand-in for bench.Worker)."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def _sparse_worker(n, k):
    g = torch.Generator().manual_seed(3)
    msg = torch.empty(2 * k, dtype=torch.int32)
    msg[:k] = torch.randn(k, generator=g).view(torch.int32)
    msg[k:] = torch.randperm(n, generator=g)[:k].to(torch.int32)
    return types.SimpleNamespace(torch=torch, op="topk", k=k, step_mode=False, msg=msg,
                                 hat=torch.randn(n, generator=g), mem=torch.randn(n, generator=g))


def test_dump_outputs_whole_arrays(tmp_path):
    w = _sparse_worker(5000, 50)
    bench.dump_outputs(w, str(tmp_path / "d"), 0, 1)
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    assert sorted(got) == ["memory", "msg_indices", "msg_values", "x_hat"]
    assert got["msg_indices"].dtype == np.float64 and got["msg_values"].dtype == np.float32
    assert np.array_equal(got["msg_indices"], w.msg[50:].numpy())
    assert np.array_equal(got["msg_values"], w.msg[:50].view(torch.float32).numpy())
    assert np.array_equal(got["x_hat"], w.hat.numpy()) and np.array_equal(got["memory"], w.mem.numpy())


def test_dump_outputs_samples_within_the_cap(tmp_path, monkeypatch):
    """Arrays over their share are cut to a seeded sample: under the cap in all, the same
    positions every run, ranks of a multi-GPU run in files of their own."""
    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)
    w = _sparse_worker(5000, 400)
    w.step_mode, w.x = True, w.hat * 2
    for d in ("a", "b"):
        bench.dump_outputs(w, str(tmp_path / d), 1, 2)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == [n + ".rank1.npy" for n in ("memory", "msg_indices", "msg_values", "x", "x_hat")]
    total = 0
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert np.array_equal(a, b)
        total += a.nbytes
    assert 2 * total <= 4000  # two ranks share the cap
    hat = np.load(tmp_path / "a" / "x_hat.rank1.npy")
    assert hat.shape == (100,) and np.isin(hat, w.hat.numpy()).all()
    assert np.array_equal(np.load(tmp_path / "a" / "x.rank1.npy"), 2 * hat)  # the same positions of x = 2 x_hat
