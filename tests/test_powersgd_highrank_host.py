"""PowerSGD at ranks 8, 16 and 32, host side (no GPU): the table against the numpy oracle,
powersgd.step_loop against the oracle's step, and the ranks that are still refused."""
import collections

import numpy as np
import pytest
import torch

import _powersgd_oracle as PO
from test_gpu_powersgd_highrank import RANKS, SHAPES
from test_powersgd_host import Identity


@pytest.mark.parametrize("r", RANKS)
def test_plan_offsets(r):
    from chocosgd_amd import codec
    plan, L = codec.LowRankPlan(SHAPES, r, "cpu"), PO.Layout(SHAPES, r)
    assert (plan.n, plan.msg1_len, plan.msg2_len) == (L.n, L.msg1_len, L.msg2_len)
    assert (plan.compressed, plan.p_off, plan.q_off) == (L.comp, L.p_off, L.q_off)
    assert plan.ws_bytes >= 4 * r * sum(-(-rows // 256) * cols for *_, rows, cols in L.matrices() if rows > 256)


@pytest.mark.parametrize("r", RANKS)
def test_step_loop_matches_the_oracle(r):
    """Two steps on fp64 CPU tensors against the numpy oracle: gradients, parameters (lr alone), e and Q."""
    from chocosgd_amd import powersgd
    L, rng = PO.Layout(SHAPES, r), np.random.RandomState(r)
    ps = [torch.nn.Parameter(torch.from_numpy(np.asarray(rng.standard_normal(s)))) for s in SHAPES]
    groups = [{"params": [p], "name": f"p{i}", "lr": 0.1, "weight_decay": 0.0, "momentum": 0.0, "dampening": 0.0,
               "nesterov": False} for i, p in enumerate(ps)]
    names = list(enumerate(f"p{i}" for i in range(len(ps))))
    comp = powersgd.PowerSGDCompressor(r, Identity(), seed=3)
    x = torch.cat([p.data.reshape(-1) for p in ps]).numpy().copy()
    e, q = np.zeros(L.n), comp.state(SHAPES, "cpu", torch.float64).q.numpy().copy()
    for _ in range(2):
        g = rng.standard_normal(L.n) * 10.0 ** rng.uniform(-3, 1, L.n)
        for p, o in zip(ps, L.off):
            p.grad = torch.from_numpy(g[o:o + p.numel()].reshape(p.shape).copy())
        assert powersgd.step_loop(comp, groups, names, collections.defaultdict(dict)) == 32 * (L.msg1_len + L.msg2_len)
        out, e, q = PO.step(L, g, e, q)
        x -= 0.1 * out
        for got, want in ((torch.cat([p.grad.reshape(-1) for p in ps]), out), (torch.cat([p.data.reshape(-1) for p in ps]), x),
                          (comp.e, e), (comp.q, q)):
            np.testing.assert_allclose(got.numpy(), want, rtol=1e-9, atol=1e-11 * np.abs(want).max())


@pytest.mark.parametrize("r", [3, 5, 64])
def test_other_ranks_are_refused(r):
    from chocosgd_amd import codec, powersgd
    with pytest.raises(RuntimeError, match="rank must be"):
        codec.LowRankPlan(SHAPES, r, "cpu")
    with pytest.raises(RuntimeError, match="rank must be"):
        powersgd.PowerSGDCompressor(r, None)
