"""PowerSGD, host side (no GPU): the compression rule at its edge, the table's offsets against the
numpy oracle, the argument checks (every refusal before any launch), fused_step's refusals, and
powersgd.step_loop against the oracle on CPU tensors."""
import collections
import ctypes

import numpy as np
import pytest
import torch

import _powersgd_oracle as PO

ERR_INVALID = -1
KERNELS = ["lowrank_project_kernel", "lowrank_orth_kernel", "lowrank_backproject_kernel", "lowrank_slabsum_kernel",
           "lowrank_decode_kernel"]
SMALL = [(9, 11), (7,), (300, 9)]


@pytest.mark.parametrize("r,shape,want", [(1, (2, 2), False), (1, (2, 3), True), (2, (4, 4), False), (2, (4, 5), True),
                                          (4, (8, 8), False), (4, (8, 9), True), (4, (2, 2, 4, 4), False),
                                          (1, (40,), False), (2, (0, 9), False)])
def test_compression_rule_edge(r, shape, want):
    from chocosgd_amd import codec, powersgd
    assert powersgd.is_compressed(shape, r) is want and PO.is_compressed(shape, r) is want
    assert codec.LowRankPlan([shape, (3,)], r, "cpu").compressed == [want, False]


@pytest.mark.parametrize("r", [1, 2, 4])
def test_plan_offsets(r):
    from chocosgd_amd import codec
    plan, L = codec.LowRankPlan(PO.SHAPES, r, "cpu"), PO.Layout(PO.SHAPES, r)
    assert (plan.n, plan.msg1_len, plan.msg2_len) == (L.n, L.msg1_len, L.msg2_len)
    assert (plan.compressed, plan.p_off, plan.q_off) == (L.comp, L.p_off, L.q_off)
    assert plan.ws_bytes >= 4 * r * sum(-(-rows // 256) * cols for *_, rows, cols in L.matrices() if rows > 256)


def _call(lib, name, plan, **kw):
    a = dict(g=0x1000, e=0x2000, q=0x3000, msg1=0x4000, msg2=0x5000, out=0x6000, ws=0x7000, ws_bytes=1 << 20,
             dev=0x8000, host=plan.plan_host, n=plan.n, rank=plan.rank, m1=plan.msg1_len, m2=plan.msg2_len, divisor=2.0)
    a.update(kw)
    a.update({k: ctypes.c_void_p(a[k]) for k in ("g", "e", "q", "msg1", "msg2", "out", "ws", "dev")})
    args = {"project": "g e q msg1 m1 m2", "orthogonalize": "msg1 m1", "backproject": "e msg1 m1 msg2 m2 ws ws_bytes",
            "decode": "e msg1 m1 msg2 m2 out divisor"}[name].split() + ["host", "dev", "n", "rank"]
    return getattr(lib, "choco_lowrank_" + name)(*[a[k] for k in args], None)


BAD = {"null g": ("project", dict(g=0), "null pointer"), "null q": ("project", dict(q=0), "null pointer"),
       "g at 4 mod 16": ("project", dict(g=0x1004), "16-byte"), "rank 3": ("project", dict(rank=3), "rank must be"),
       "rank of another table": ("decode", dict(rank=4), "built for rank"), "another n": ("orthogonalize", dict(n=7), "built for n"),
       "null table": ("orthogonalize", dict(host=None), "null table"), "null device table": ("backproject", dict(dev=0), "null table"),
       "short message 1": ("orthogonalize", dict(m1=5), "message 1"), "long message 2": ("backproject", dict(m2=999), "message 2"),
       "null msg1": ("orthogonalize", dict(msg1=0), "null pointer"), "null msg2": ("backproject", dict(msg2=0), "null pointer"),
       "small workspace": ("backproject", dict(ws_bytes=16), "workspace too small"), "divisor 0": ("decode", dict(divisor=0.0), "divisor"),
       "divisor -2": ("decode", dict(divisor=-2.0), "divisor"), "null flat_out": ("decode", dict(out=0), "null pointer"),
       "e at 8 mod 16": ("decode", dict(e=0x2008), "16-byte")}


@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_arguments_are_rejected(case):
    """The made-up device pointers are never dereferenced: every case is refused before the launch."""
    from chocosgd_amd import _lib, codec
    name, kw, msg = BAD[case]
    plan = codec.LowRankPlan(SMALL, 2, "cpu")
    before = [codec.launch_count(k) for k in KERNELS]
    assert _call(_lib.load(), name, plan, **kw) == ERR_INVALID
    assert msg in _lib.last_error(), _lib.last_error()
    assert [codec.launch_count(k) for k in KERNELS] == before
    p_i64 = ctypes.POINTER(ctypes.c_int64)
    assert _lib.load().choco_lowrank_plan_len(ctypes.cast(None, p_i64), ctypes.cast(None, p_i64), 1, 2) < 0
    with pytest.raises(RuntimeError, match="rank must be"):
        codec.LowRankPlan(SMALL, 3, "cpu")


@pytest.mark.parametrize("kw", [dict(master=object()), dict(clip_norm=1.0), dict(loss_scale=object()), dict(rounding=object())])
def test_fused_step_refuses(kw):
    from chocosgd_amd import powersgd
    with pytest.raises(RuntimeError, match="not supported"):
        powersgd.fused_step(powersgd.PowerSGDCompressor(2, None), [], [], {}, **kw)
    with pytest.raises(RuntimeError, match="rank must be"):
        powersgd.PowerSGDCompressor(3, None)


class Identity:
    world_size = 1.0

    def _agg(self, data, op=None, distributed=True):
        assert op == "sum"
        return data


@pytest.mark.parametrize("r", [1, 2, 4])
def test_step_loop_matches_the_oracle(r):
    """Two steps on fp64 CPU tensors against the numpy oracle: gradients (the decoded average),
    parameters (lr alone), e and Q; another layout is refused."""
    from chocosgd_amd import powersgd
    shapes = [s for s in PO.SHAPES if PO.numel(s) < 3000]
    L, rng = PO.Layout(shapes, r), np.random.RandomState(r)
    ps = [torch.nn.Parameter(torch.from_numpy(np.asarray(rng.standard_normal(s)))) for s in shapes]
    groups = [{"params": [p], "name": f"p{i}", "lr": 0.1, "weight_decay": 0.0, "momentum": 0.0, "dampening": 0.0,
               "nesterov": False} for i, p in enumerate(ps)]
    names = list(enumerate(f"p{i}" for i in range(len(ps))))
    comp = powersgd.PowerSGDCompressor(r, Identity(), seed=3)
    x = torch.cat([p.data.reshape(-1) for p in ps]).numpy().copy()
    e = np.zeros(L.n)
    q = comp.state(shapes, "cpu", torch.float64).q.numpy().copy()
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
    with pytest.raises(RuntimeError, match="another layout"):
        comp.state(shapes[:-1], "cpu", torch.float64)
