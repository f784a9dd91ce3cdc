"""PowerSGD on the device: codec.LowRankPlan's launches against fp64 numpy within forward error bounds
taken from the reference's own absolute sums, the error memory bit for bit, orthogonalise and
powersgd.fused_step within four times the fp32 restatement's own distance from fp64, a gradient of
rank <= r (nothing is lost), and the four calls on a delayed side stream."""
import collections

import numpy as np
import pytest
import torch

import _powersgd_oracle as PO
import _streams as ST
from conftest import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.0
RANKS = [1, 2, 4]
RESNET20ISH = [(16, 3, 3, 3), (16,), (16,), (16, 16, 3, 3), (16,), (32, 16, 3, 3), (32,), (32, 16, 1, 1), (64, 32, 3, 3),
               (64,), (64, 64, 3, 3), (10, 64), (10,)]
ORTH_SHAPES = [(64, 147), (7,), (300, 9), (33, 40), (2049, 5)]  # rows >= 8 r; 2049: one over the staged rows
KERNELS = ["lowrank_project_kernel", "lowrank_orth_kernel", "lowrank_backproject_kernel", "lowrank_slabsum_kernel",
           "lowrank_decode_kernel"]


def spread(rng, n):
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def setup(r, shapes=PO.SHAPES, seed=0):
    from chocosgd_amd import codec
    L, rng = PO.Layout(shapes, r), np.random.RandomState(seed + r)
    a = {k: spread(rng, m) for k, m in (("g", L.n), ("e", L.n), ("q", L.msg2_len), ("msg1", L.msg1_len), ("msg2", L.msg2_len))}
    return codec.LowRankPlan(shapes, r, DEV), L, a


def bounded(got, A, B, terms):
    """|got - A B| <= (terms + 2) 2^-24 |A| |B|: a length-`terms` fp32 dot product in any order, plus an input rounding."""
    A, B = A.astype(np.float64), B.astype(np.float64)
    return np.all(np.abs(got - A @ B) <= (terms + 2) * 2.0 ** -24 * (np.abs(A) @ np.abs(B)))


@pytest.mark.parametrize("r", RANKS)
def test_project(r):
    plan, L, a = setup(r)
    runs = []
    for _ in range(2):
        e, msg1 = dev(a["e"]), torch.full((L.msg1_len,), SENTINEL, device=DEV)
        plan.project(dev(a["g"]), e, dev(a["q"]), msg1)
        runs.append((e.cpu().numpy(), msg1.cpu().numpy()))
    (e, msg1), M = runs[0], a["e"].copy()
    for f, ps, qs, rows, cols in L.matrices():
        M[f] = a["g"][f] + a["e"][f]
        assert bounded(msg1[ps].reshape(rows, r), M[f].reshape(rows, cols), a["q"][qs].reshape(cols, r), cols), (rows, cols)
    assert same_bits(e, M), "M over e; the uncompressed tensors' e untouched"
    assert all(same_bits(msg1[t], a["g"][f]) for f, t in L.tails())
    assert same_bits(runs[1][0], e) and same_bits(runs[1][1], msg1), "the same bits twice"


@pytest.mark.parametrize("r", RANKS)
def test_backproject(r):
    plan, L, a = setup(r, seed=10)
    runs = []
    for _ in range(2):
        msg2 = torch.full((L.msg2_len,), SENTINEL, device=DEV)
        plan.backproject(dev(a["e"]), dev(a["msg1"]), msg2)
        runs.append(msg2.cpu().numpy())
    for f, ps, qs, rows, cols in L.matrices():
        assert bounded(runs[0][qs].reshape(cols, r), a["e"][f].reshape(rows, cols).T, a["msg1"][ps].reshape(rows, r), rows), (rows, cols)
    assert same_bits(runs[0], runs[1])


@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("r", RANKS)
def test_decode(r, W):
    plan, L, a = setup(r, seed=20)
    for f, _ in L.tails():
        a["e"][f] = SENTINEL
    e, out = dev(a["e"]), torch.full((L.n,), SENTINEL, device=DEV)
    plan.decode(e, dev(a["msg1"]), dev(a["msg2"]), out, float(W))
    e, out, want_e = e.cpu().numpy(), out.cpu().numpy(), a["e"].copy()
    for f, ps, qs, rows, cols in L.matrices():
        assert bounded(out[f].reshape(rows, cols), a["msg1"][ps].reshape(rows, r), a["msg2"][qs].reshape(cols, r).T, r - 1), (rows, cols)
        want_e[f] = a["e"][f] - out[f] / np.float32(W)
    assert same_bits(e, want_e), "e = fl(M - fl(out / W)) from the out the kernel wrote; sentinels untouched"
    assert all(same_bits(out[f], a["msg1"][t]) for f, t in L.tails())


@pytest.mark.parametrize("r", RANKS)
def test_orthogonalize(r):
    from chocosgd_amd import codec
    plan, L = codec.LowRankPlan(ORTH_SHAPES, r, DEV), PO.Layout(ORTH_SHAPES, r)
    x = np.random.RandomState(r).standard_normal(L.msg1_len).astype(np.float32)
    msg1 = dev(x)
    plan.orthogonalize(msg1)
    got, d, dist = msg1.cpu().numpy(), 0.0, 0.0
    for _, ps, _, rows, _ in L.matrices():
        want = PO.orthogonalize(x[ps].reshape(rows, r))
        d = max(d, np.abs(PO.orthogonalize(x[ps].reshape(rows, r), np.float32) - want).max())
        dist = max(dist, np.abs(got[ps].reshape(rows, r) - want).max())
    print(f"orthogonalise r={r}: fp32 restatement d = {d:.3g}, kernel distance {dist:.3g}")
    assert dist <= 4 * d
    assert same_bits(got[L.msg1_len - 7:], x[L.msg1_len - 7:]), "the tail is not touched"
    # a zero matrix, and a zero column among Gaussian ones: finite, zeros stay zeros
    ps = [m[1] for m in L.matrices()]
    x[ps[0]] = 0.0
    x[ps[1]].reshape(-1, r)[:, r - 1] = 0.0
    msg1 = dev(x)
    plan.orthogonalize(msg1)
    got = msg1.cpu().numpy()
    assert np.isfinite(got).all() and not got[ps[0]].any() and not got[ps[1]].reshape(-1, r)[:, r - 1].any()


class Loopback:
    """rank 0's all-reduce: its own message plus W - 1 prepared peer messages (the same fp32
    values for every model that draws them in the same order)."""

    def __init__(self, world, seed):
        self.world_size, self.rng = float(world), np.random.RandomState(seed)

    def _agg(self, data, op=None, distributed=True):
        assert op == "sum"
        for _ in range(int(self.world_size) - 1):
            data = data + torch.from_numpy(self.rng.standard_normal(data.numel()).astype(np.float32)).to(data.device, data.dtype)
        return data


def model(shapes, device, dtype, momentum=0.9):
    g = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).to(device, dtype)) for s in shapes]
    groups = [{"params": [p], "name": f"p{i}", "lr": 0.01 * (i % 3 + 1), "weight_decay": 1e-4, "momentum": momentum,
               "dampening": 0.0, "nesterov": False} for i, p in enumerate(ps)]
    return ps, groups, list(enumerate(f"p{i}" for i in range(len(ps)))), collections.defaultdict(dict)


def set_grads(ps, L, flat):
    for p, o in zip(ps, L.off):
        p.grad = torch.from_numpy(flat[o:o + p.numel()].reshape(p.shape).copy()).to(p.device, p.dtype)


def cat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts]).double().cpu().numpy()


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("layout", ["kernel tests", "resnet20-like"])
def test_fused_step_vs_loop(layout, r, world):
    from chocosgd_amd import codec, powersgd
    shapes = PO.SHAPES if layout == "kernel tests" else RESNET20ISH
    L, rng = PO.Layout(shapes, r), np.random.RandomState(world)
    runs = [(powersgd.fused_step, DEV, torch.float32), (powersgd.step_loop, "cpu", torch.float64),
            (powersgd.step_loop, "cpu", torch.float32)]
    models = [model(shapes, d, dt) for _, d, dt in runs]
    comps = [powersgd.PowerSGDCompressor(r, Loopback(world, 7), seed=1) for _ in runs]
    launches = [1, 1, 1, int(any(rows > 256 for *_, rows, _ in L.matrices())), 1]
    for step in range(2):  # the second step reads e, the warm Q and the momentum buffers
        flat = spread(rng, L.n)
        for (fn, _, _), (ps, groups, names, state), comp in zip(runs, models, comps):
            set_grads(ps, L, flat)
            c0 = [codec.launch_count(k) for k in KERNELS]
            assert fn(comp, groups, names, state) == 32 * (L.msg1_len + L.msg2_len)
            assert [codec.launch_count(k) - c for k, c in zip(KERNELS, c0)] == (launches if fn is powersgd.fused_step else [0] * 5)
        for name, get in (("params", lambda i: cat(models[i][0])), ("e", lambda i: cat([comps[i].e])),
                          ("Q", lambda i: cat([comps[i].q]))):
            d, dist = np.abs(get(2) - get(1)).max(), np.abs(get(0) - get(1)).max()
            print(f"{layout} r={r} W={world} step {step} {name}: d = {d:.3g}, fused distance {dist:.3g}")
            assert dist <= 4 * d, (name, step)


@pytest.mark.parametrize("r", RANKS)
def test_low_rank_gradient_loses_nothing(r):
    """Gradients of rank <= r exactly (integer factors: the products are exact in fp32)."""
    from chocosgd_amd import powersgd, utils
    shapes = [(64, 147), (7,), (300, 9), (33, 40)]
    L, rng = PO.Layout(shapes, r), np.random.RandomState(r)
    flat = spread(rng, L.n)
    for f, _, _, rows, cols in L.matrices():
        flat[f] = (rng.randint(-8, 9, (rows, r)) @ rng.randint(-8, 9, (r, cols))).reshape(-1)
    q = powersgd.PowerSGDCompressor(r, None, seed=1).state(shapes, "cpu").q.numpy()
    e64, e32 = (PO.step(L, flat, np.zeros(L.n), q, dtype=dt)[1] for dt in (np.float64, np.float32))
    d = np.abs(e32 - e64).max()
    comp = powersgd.PowerSGDCompressor(r, Loopback(1, 0), seed=1)
    (pa, ga, na, sa), (pb, gb, nb, sb) = (model(shapes, DEV, torch.float32, momentum=0.0) for _ in range(2))
    set_grads(pa, L, flat)
    set_grads(pb, L, flat)
    powersgd.fused_step(comp, ga, na, sa)
    utils.allreduce_sgd_step(gb, nb, sb, comp.aggregator_fn)
    print(f"low-rank gradient r={r}: d = {d:.3g}, max|e| = {comp.e.abs().max().item():.3g}")
    assert comp.e.abs().max().item() <= 4 * d and np.abs(cat(pa) - cat(pb)).max() <= 4 * d


@pytest.mark.parametrize("call", ["project", "orthogonalize", "backproject", "decode"])
def test_streams(call):
    plan, L, a = setup(2)
    names, nout = {"project": (("g", "e", "q"), L.msg1_len), "orthogonalize": (("msg1",), 0),
                   "backproject": (("e", "msg1"), L.msg2_len), "decode": (("e", "msg1", "msg2"), L.n)}[call]
    true = {k: dev(a[k]) for k in names}
    work, poison = {k: t.clone() for k, t in true.items()}, {k: t * 0.5 + 1.0 for k, t in true.items()}
    outs = [torch.empty(nout, device=DEV)] if nout else []
    fn = {"project": lambda: plan.project(work["g"], work["e"], work["q"], outs[0]),
          "orthogonalize": lambda: plan.orthogonalize(work["msg1"]),
          "backproject": lambda: plan.backproject(work["e"], work["msg1"], outs[0]),
          "decode": lambda: plan.decode(work["e"], work["msg1"], work["msg2"], outs[0], 3.0)}[call]
    fn()  # on the null stream, from the true inputs: the same bits are expected on the side stream
    want = [t.clone() for t in list(work.values()) + outs]
    _, got_work, got_outs = ST.run(fn, work, true, poison, outs=outs, family="powersgd", case=call)
    assert all(torch.equal(g, w) for g, w in zip(list(got_work.values()) + got_outs, want))
