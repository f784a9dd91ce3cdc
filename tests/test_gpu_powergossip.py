"""PowerGossip on the device: codec.LowRankGossipPlan's launches, batched over a worker's edges, against
fp64 numpy (test_gpu_powersgd's forward error bound), the bit-level contract between the two ends of an
edge, and powergossip.fused_step against step_loop."""
import numpy as np
import pytest
import torch

import _powersgd_oracle as PO
from conftest import same_bits
from test_gpu_powersgd import ORTH_SHAPES, RESNET20ISH, bounded, cat, dev, model, set_grads, spread

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.0
CASES = [(1, 2), (2, 2), (4, 2), (1, 3), (2, 4), (1, 8)]  # (r, E)
SHAPES = PO.SHAPES + [(5, 1025)]  # 2049 / 1025: one over the column block up to K = 4 / at K = 8
U = 2.0 ** -24


def setup(r, E, shapes=SHAPES, seed=0):
    """The plan, the layout, lo_mask (alternating ends), weights (exact in fp32) and spread inputs per buffer."""
    from chocosgd_amd import codec
    L, rng = PO.Layout(shapes, r), np.random.RandomState(seed + 10 * r + E)
    pt = sum(rows * r for rows, _ in L.rc)
    a = {k: spread(rng, E * m).reshape(E, m) for k, m in (("q", L.msg2_len), ("recv1", L.msg1_len), ("phat", pt),
                                                         ("own2", L.msg2_len), ("recv2", L.msg2_len), ("dq", L.msg2_len))}
    a["x"] = spread(rng, L.n)
    return codec.LowRankGossipPlan(shapes, r, E, DEV), L, 0x55 & ((1 << E) - 1), [2.0 ** -(3 + e % 2) for e in range(E)], a


def sentinel(E, m):
    return torch.full((E * m,), SENTINEL, device=DEV)


def flat(a):
    return dev(a.reshape(-1))


@pytest.mark.parametrize("r,E", CASES)
def test_project(r, E):
    plan, L, _, _, a = setup(r, E)
    x, runs = dev(a["x"]), []
    for _ in range(2):
        msg1 = sentinel(E, L.msg1_len)
        plan.project(x, flat(a["q"]), msg1)
        runs.append(msg1.cpu().numpy().reshape(E, -1))
    for e in range(E):
        for f, ps, qs, rows, cols in L.matrices():
            assert bounded(runs[0][e][ps].reshape(rows, r), a["x"][f].reshape(rows, cols), a["q"][e][qs].reshape(cols, r), cols), (e, rows, cols)
        assert all(same_bits(runs[0][e][t], a["x"][f]) for f, t in L.tails())
    assert same_bits(x.cpu().numpy(), a["x"]) and same_bits(runs[0], runs[1]), "x untouched; the same bits twice"


@pytest.mark.parametrize("r,E", CASES)
def test_backproject(r, E):
    plan, L, _, _, a = setup(r, E, seed=1)
    runs = []
    for _ in range(2):
        msg2 = sentinel(E, L.msg2_len)
        plan.backproject(dev(a["x"]), flat(a["phat"]), msg2)
        runs.append(msg2.cpu().numpy().reshape(E, -1))
    for e in range(E):
        for f, ps, qs, rows, cols in L.matrices():
            assert bounded(runs[0][e][qs].reshape(cols, r), a["x"][f].reshape(rows, cols).T, a["phat"][e][ps].reshape(rows, r), rows), (e, rows, cols)
    assert same_bits(runs[0], runs[1])


@pytest.mark.parametrize("r,E", CASES)
def test_orthogonalize(r, E):
    plan, L, mask, _, _ = setup(r, E, ORTH_SHAPES)
    rng, pt = np.random.RandomState(r + E), plan.p_total
    own, recv = (rng.standard_normal((E, L.msg1_len)).astype(np.float32) for _ in range(2))
    out = [sentinel(E, pt) for _ in range(3)]
    plan.orthogonalize(flat(own), flat(recv), out[0], mask)
    plan.orthogonalize(flat(recv), flat(own), out[1], ~mask & 0xff)  # the same pairs from the other ends
    plan.orthogonalize(flat(own), flat(own), out[2], mask)
    got, d, dist = out[0].cpu().numpy().reshape(E, pt), 0.0, 0.0
    for e in range(E):
        dP = own[e] - recv[e] if mask >> e & 1 else recv[e] - own[e]
        for _, ps, _, rows, _ in L.matrices():
            want = PO.orthogonalize(dP[ps].reshape(rows, r))
            d = max(d, np.abs(PO.orthogonalize(dP[ps].reshape(rows, r), np.float32) - want).max())
            dist = max(dist, np.abs(got[e][ps].reshape(rows, r) - want).max())
    print(f"gossip orthogonalise r={r} E={E}: fp32 restatement d = {d:.3g}, kernel distance {dist:.3g}")
    assert dist <= 4 * d
    assert torch.equal(out[0], out[1]), "bit-equal at both ends of every edge"
    assert not out[2].any(), "a zero difference gives zeros"


@pytest.mark.parametrize("r,E", CASES)
def test_diff(r, E):
    plan, L, mask, _, a = setup(r, E, seed=2)
    zero = [m[2] for m in L.matrices()][1]
    a["recv2"][0][zero] = a["own2"][0][zero]  # edge 0 agrees exactly on one matrix
    q, dq = flat(a["q"]), sentinel(E, L.msg2_len)
    plan.diff(flat(a["own2"]), flat(a["recv2"]), q, dq, mask)
    want = np.stack([a["own2"][e] - a["recv2"][e] if mask >> e & 1 else a["recv2"][e] - a["own2"][e] for e in range(E)])
    assert same_bits(dq.cpu().numpy().reshape(E, -1), want)
    want[0][zero] = a["q"][0][zero]
    assert same_bits(q.cpu().numpy().reshape(E, -1), want), "the all-zero matrix keeps its old Q bit for bit"


@pytest.mark.parametrize("r,E", CASES)
def test_apply(r, E):
    plan, L, mask, w, a = setup(r, E, seed=3)
    x = dev(a["x"])
    plan.apply(x, flat(a["phat"]), flat(a["dq"]), flat(a["recv1"]), w, mask)
    got, x0 = x.cpu().numpy().astype(np.float64), a["x"].astype(np.float64)
    for f, ps, qs, rows, cols in L.matrices():
        P = [a["phat"][e][ps].reshape(rows, r).astype(np.float64) for e in range(E)]
        Q = [a["dq"][e][qs].reshape(cols, r).astype(np.float64) for e in range(E)]
        want = x0[f].reshape(rows, cols) + sum((-w[e] if mask >> e & 1 else w[e]) * (P[e] @ Q[e].T) for e in range(E))
        mag = [w[e] * (np.abs(P[e]) @ np.abs(Q[e]).T) for e in range(E)]  # the product bound, terms = r - 1, scaled by |c_e|
        bound = (r + 1) * U * sum(mag) + (E + 1) * U * (np.abs(x0[f]).reshape(rows, cols) + sum(mag))
        assert np.all(np.abs(got[f].reshape(rows, cols) - want) <= bound), (rows, cols)
    for f, t in L.tails():  # the plain mix: one rounding per subtraction, exact weights, E adds
        want = x0[f] + sum(w[e] * (a["recv1"][e][t].astype(np.float64) - x0[f]) for e in range(E))
        mag = np.abs(x0[f]) + sum(w[e] * (np.abs(a["recv1"][e][t]) + np.abs(x0[f])) for e in range(E))
        assert np.all(np.abs(got[f] - want) <= (E + 2) * U * mag)


@pytest.mark.parametrize("r", [1, 2, 4])
def test_two_endpoints(r):
    """Workers A (rank 0, the low end) and B (rank 1) of one edge, two steps by hand, the messages swapped here."""
    plan, L, _, _, a = setup(r, 1, seed=4)
    b = setup(r, 1, seed=5)[4]
    X, Q = [dev(a["x"]), dev(b["x"])], [flat(a["q"]), flat(a["q"])]
    total, budget = a["x"].astype(np.float64) + b["x"].astype(np.float64), 0.0
    for step in (1, 2):
        m1, ph, m2, dq = ([torch.empty(m, device=DEV) for _ in range(2)] for m in (L.msg1_len, plan.p_total, L.msg2_len, L.msg2_len))
        for i in (0, 1):
            plan.project(X[i], Q[i], m1[i])
        for i in (0, 1):
            plan.orthogonalize(m1[i], m1[1 - i], ph[i], 1 - i)
            plan.backproject(X[i], ph[i], m2[i])
        for i in (0, 1):
            plan.diff(m2[i], m2[1 - i], Q[i], dq[i], 1 - i)
            plan.apply(X[i], ph[i], dq[i], m1[1 - i], [0.5], 1 - i)
        assert torch.equal(ph[0], ph[1]) and torch.equal(dq[0], dq[1]) and torch.equal(Q[0], Q[1]), step
        xa, xb = (t.cpu().numpy() for t in X)
        budget = budget + 2.0 * np.spacing(np.maximum(np.abs(xa), np.abs(xb)))  # 2 ulp per element per step
        assert np.all(np.abs(xa.astype(np.float64) + xb - total) <= budget), step
    assert not torch.equal(Q[0], flat(a["q"]))


# odd column counts (rows off the 16-byte grid: head and tail run); 2049 columns, one over the LDS column block;
# 257 rows, two slabs (the slab sum runs); one uncompressed tensor
ONE_EDGE_SHAPES = [(7,), (9, 11), (7, 257), (5, 5), (5, 2049), (257, 6)]


@pytest.mark.parametrize("r", [1, 2, 4])
def test_one_edge_is_powersgd(r):
    """At one edge PowerGossip's passes are PowerSGD's (codec.LowRankPlan on the same table): the same row walk, the
    same back-project and slab-sum kernels, the same product chain, so the same bits."""
    gossip, L, _, _, a = setup(r, 1, ONE_EDGE_SHAPES, seed=6)
    sgd, x, q, phat, dq, recv1 = gossip.table, a["x"], a["q"][0], a["phat"][0], a["dq"][0], a["recv1"][0]
    msg1 = np.concatenate([phat, recv1[gossip.p_total:]])  # [P^ | anything]
    got, want = sentinel(1, L.msg1_len), sentinel(1, L.msg1_len)
    gossip.project(dev(x), dev(q), got)
    sgd.project(dev(x), torch.zeros(L.n, device=DEV), dev(q), want)  # M = x + 0
    assert same_bits(got.cpu().numpy(), want.cpu().numpy()), "project: the whole of message 1"
    got, want = sentinel(1, L.msg2_len), sentinel(1, L.msg2_len)
    gossip.backproject(dev(x), dev(phat), got)
    sgd.backproject(dev(x), dev(msg1), want)
    assert same_bits(got.cpu().numpy(), want.cpu().numpy()), "back-project"
    # apply at the low end with weight 1 (c = -1) against decode with divisor 1: -1 * o and o / 1 are exact
    got, want = dev(x), dev(x)
    gossip.apply(got, dev(phat), dev(dq), dev(recv1), [1.0], 1)
    sgd.decode(want, dev(msg1), dev(dq), sentinel(1, L.n), 1.0)
    got, want = got.cpu().numpy(), want.cpu().numpy()
    assert all(same_bits(got[f], want[f]) for f, *_ in L.matrices()), "apply against decode, the compressed matrices"


class Peers:
    """Worker 1's exchange: prepared Gaussian peer messages, the same values for every model."""
    rank = 1

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)

    def exchange_edges(self, messages, out=None):
        got = {j: torch.from_numpy(self.rng.standard_normal(t.numel())).to(t.device, t.dtype) for j, t in messages.items()}
        return got if out is None else {j: out[j].copy_(t) for j, t in got.items()}


@pytest.mark.parametrize("r,E", CASES)
def test_fused_step_vs_loop(r, E):
    from chocosgd_amd import codec, powergossip
    L, rng = PO.Layout(RESNET20ISH, r), np.random.RandomState(E)
    info = {j: 1.0 / (E + 1) for j in range(E + 1)}  # worker 1: the high end of edge (0, 1), the low end of the others
    runs = [(powergossip.fused_step, DEV, torch.float32), (powergossip.step_loop, "cpu", torch.float64),
            (powergossip.step_loop, "cpu", torch.float32), (powergossip.fused_step, DEV, torch.bfloat16),
            (powergossip.step_loop, "cpu", torch.float64)]
    models = [model(RESNET20ISH, d, dt, momentum=0.9 if i < 3 else 0.0) for i, (_, d, dt) in enumerate(runs)]
    # The bf16 copy's own fp64 reference starts from its values, and both take lr = 0: a 16-bit model's local update
    # packs the ROUNDED new parameters (choco_params_sgd, as in dpsgd_step), and where that rounding falls is not this
    # step's business -- with the identity update X is the widened model exactly, on the device and in the reference.
    for p16, p64, g16, g64 in zip(models[3][0], models[4][0], models[3][1], models[4][1]):
        p64.data.copy_(p16.data.double())
        g16["lr"] = g64["lr"] = 0.0
    comps = [powergossip.PowerGossipCompressor(r, Peers(7), info, seed=1) for _ in runs]
    for step in range(2):  # the second step reads the warm Q and the momentum buffers
        grads = spread(rng, L.n)
        for i, ((fn, _, _), (ps, groups, names, state), comp) in enumerate(zip(runs, models, comps)):
            if i >= 3 and step:
                continue  # the bf16 copy: one step (its parameters are rounded, the reference's are not)
            set_grads(ps, L, grads)
            c0 = codec.launch_count("lowrank_gossip_apply_kernel")
            assert fn(comp, groups, names, state) == 32 * E * (L.msg1_len + L.msg2_len)
            assert codec.launch_count("lowrank_gossip_apply_kernel") - c0 == (fn is powergossip.fused_step)
        for name, get in (("params", lambda i: cat(models[i][0])), ("Q", lambda i: cat([comps[i].q]))):
            d, dist = np.abs(get(2) - get(1)).max(), np.abs(get(0) - get(1)).max()
            print(f"r={r} E={E} step {step} {name}: d = {d:.3g}, fused distance {dist:.3g}")
            assert dist <= 4 * d, (name, step)
            if name == "params" and step == 0:  # bf16: the fp32 X within 4 d, then one rounding to 8 bits
                assert np.all(np.abs(get(3) - get(4)) <= 4 * d + 2.0 ** -8 * np.abs(get(4)))


@pytest.mark.parametrize("kw", [dict(master=object()), dict(clip_norm=1.0), dict(loss_scale=object()), dict(rounding=object())])
def test_fused_step_refuses(kw):
    from chocosgd_amd import powergossip
    with pytest.raises(RuntimeError, match="not supported"):
        powergossip.fused_step(powergossip.PowerGossipCompressor(2, Peers(0), {0: 0.5, 1: 0.5}), [], [], {}, **kw)
