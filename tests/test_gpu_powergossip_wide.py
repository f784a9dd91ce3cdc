"""PowerGossip beyond E r = 8 on the device (csrc/lowrank_gossip_mfma.hip): codec.LowRankGossipWidePlan's launches
against fp64 numpy on test_gpu_powersgd_highrank's layout, the bit-level contract between the two ends of an edge,
and powergossip.fused_step against step_loop.  (r, E): widths 12, 16, 14, 9 (more than 8 edges), 8 at rank 8, 16 at
rank 8, 28 and 32 (two result tiles)."""
import numpy as np
import pytest
import torch

import _powersgd_oracle as PO
from conftest import same_bits
from test_gpu_powergossip import Peers
from test_gpu_powersgd import RESNET20ISH, cat, dev, model, set_grads, spread
from test_gpu_powersgd_highrank import SHAPES, ratio

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.0
CASES = [(4, 3), (4, 4), (2, 7), (1, 9), (8, 1), (8, 2), (4, 7), (16, 2)]  # (r, E)
U = 2.0 ** -24


def setup(r, E, seed=0):
    """The plan, the layout, lo_mask (alternating ends), weights (exact in fp32) and spread inputs per buffer."""
    from chocosgd_amd import codec
    L, rng = PO.Layout(SHAPES, r), np.random.RandomState(seed + 10 * r + E)
    pt = sum(rows * r for rows, _ in L.rc)
    a = {k: spread(rng, E * m).reshape(E, m) for k, m in (("q", L.msg2_len), ("recv1", L.msg1_len), ("phat", pt),
                                                         ("dq", L.msg2_len))}
    a["x"] = spread(rng, L.n)
    return codec.LowRankGossipWidePlan(SHAPES, r, E, DEV), L, 0x55555555 & ((1 << E) - 1), [2.0 ** -(3 + e % 2) for e in range(E)], a


def guarded(E, m):
    """A sentinel-filled buffer of E + 1 edges: the launch gets the first E, a padded column stored shows in the last."""
    buf = torch.full(((E + 1) * m,), SENTINEL, device=DEV)
    return buf, buf[:E * m]


def flat(a):
    return dev(a.reshape(-1))


@pytest.mark.parametrize("r,E", CASES)
def test_project(r, E):
    plan, L, _, _, a = setup(r, E)
    x, runs, worst = dev(a["x"]), [], 0.0
    for _ in range(2):
        buf, msg1 = guarded(E, L.msg1_len)
        plan.project(x, flat(a["q"]), msg1)
        runs.append(buf.cpu().numpy().reshape(E + 1, -1))
    for e in range(E):
        for f, ps, qs, rows, cols in L.matrices():
            worst = max(worst, ratio(runs[0][e][ps].reshape(rows, r), a["x"][f].reshape(rows, cols), a["q"][e][qs].reshape(cols, r), cols))
        assert all(same_bits(runs[0][e][t], a["x"][f]) for f, t in L.tails())
    print(f"wide project r={r} E={E}: worst error / bound = {worst:.3g}")
    assert worst <= 1.0
    assert np.all(runs[0][E] == SENTINEL), "nothing stored past the E edges"
    assert same_bits(x.cpu().numpy(), a["x"]) and same_bits(runs[0], runs[1]), "x untouched; the same bits twice"


@pytest.mark.parametrize("r,E", CASES)
def test_backproject(r, E):
    plan, L, _, _, a = setup(r, E, seed=1)
    x, runs, worst = dev(a["x"]), [], 0.0
    for _ in range(2):
        buf, msg2 = guarded(E, L.msg2_len)
        plan.backproject(x, flat(a["phat"]), msg2)
        runs.append(buf.cpu().numpy().reshape(E + 1, -1))
    for e in range(E):
        for f, ps, qs, rows, cols in L.matrices():
            worst = max(worst, ratio(runs[0][e][qs].reshape(cols, r), a["x"][f].reshape(rows, cols).T, a["phat"][e][ps].reshape(rows, r), rows))
    print(f"wide back-project r={r} E={E}: worst error / bound = {worst:.3g}")
    assert worst <= 1.0
    assert np.all(runs[0][E] == SENTINEL), "nothing stored past the E edges"
    assert same_bits(x.cpu().numpy(), a["x"]) and same_bits(runs[0], runs[1]), "x untouched; the same bits twice"


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
        mag = sum(w[e] * (np.abs(P[e]) @ np.abs(Q[e]).T) for e in range(E))
        # one rounding of c p, an E r-term dot product in any order, the final add
        bound = (E * r + 3) * U * mag + U * (np.abs(x0[f]).reshape(rows, cols) + mag)
        assert np.all(np.abs(got[f].reshape(rows, cols) - want) <= bound), (rows, cols)
    for f, t in L.tails():  # the plain mix: one rounding per subtraction, exact weights, E adds
        want = x0[f] + sum(w[e] * (a["recv1"][e][t].astype(np.float64) - x0[f]) for e in range(E))
        mag = np.abs(x0[f]) + sum(w[e] * (np.abs(a["recv1"][e][t]) + np.abs(x0[f])) for e in range(E))
        assert np.all(np.abs(got[f] - want) <= (E + 2) * U * mag)


@pytest.mark.parametrize("r,E", [(4, 4), (8, 2), (16, 2)])
def test_orthogonalize_and_diff(r, E):
    plan, L, mask, _, a = setup(r, E, seed=2)
    rng, pt = np.random.RandomState(r + E), plan.p_total
    own, recv = (rng.standard_normal((E, L.msg1_len)).astype(np.float32) for _ in range(2))
    out = [torch.full((E * pt,), SENTINEL, device=DEV) for _ in range(3)]
    plan.orthogonalize(flat(own), flat(recv), out[0], mask)
    plan.orthogonalize(flat(recv), flat(own), out[1], ~mask & 0xffffffff)  # the same pairs from the other ends
    plan.orthogonalize(flat(own), flat(own), out[2], mask)
    got, d, dist = out[0].cpu().numpy().reshape(E, pt), 0.0, 0.0
    for e in range(E):
        dP = own[e] - recv[e] if mask >> e & 1 else recv[e] - own[e]
        for _, ps, _, rows, _ in L.matrices():
            want = PO.orthogonalize(dP[ps].reshape(rows, r))
            d = max(d, np.abs(PO.orthogonalize(dP[ps].reshape(rows, r), np.float32) - want).max())
            dist = max(dist, np.abs(got[e][ps].reshape(rows, r) - want).max())
    print(f"wide orthogonalise r={r} E={E}: fp32 restatement d = {d:.3g}, kernel distance {dist:.3g}")
    assert dist <= 4 * d
    assert torch.equal(out[0], out[1]), "bit-equal at both ends of every edge"
    assert not out[2].any(), "a zero difference gives zeros"
    own2, recv2 = a["dq"], a["q"].copy()  # diff: two spread message 2s, edge 0 agreeing exactly on one matrix
    zero = [m[2] for m in L.matrices()][1]
    recv2[0][zero] = own2[0][zero]
    q, dq = flat(a["q"] + 1.0), torch.full((E * L.msg2_len,), SENTINEL, device=DEV)
    plan.diff(flat(own2), flat(recv2), q, dq, mask)
    want = np.stack([own2[e] - recv2[e] if mask >> e & 1 else recv2[e] - own2[e] for e in range(E)])
    assert same_bits(dq.cpu().numpy().reshape(E, -1), want)
    want[0][zero] = (a["q"] + 1.0)[0][zero]
    assert same_bits(q.cpu().numpy().reshape(E, -1), want), "the all-zero matrix keeps its old Q bit for bit"


@pytest.mark.parametrize("r,E", [(8, 1), (16, 1), (4, 4), (2, 7)])
def test_two_endpoints(r, E):
    """Worker A holds E edges, edge 0 (to B) as its low end; B holds the same edges from their other ends.  Two steps by
    hand, every edge's messages swapped here.  Both ends feed the matrix instruction exactly negated operands, so the
    updates are exact negations: X_A + X_B moves by the two final adds' roundings alone."""
    plan, L, _, _, a = setup(r, E, seed=4)
    b, mask = setup(r, E, seed=5)[4], [0x55555555 & ((1 << E) - 1), 0xaaaaaaaa & ((1 << E) - 1)]
    X, Q, w = [dev(a["x"]), dev(b["x"])], [flat(a["q"]), flat(a["q"])], [0.5] if E == 1 else [0.125] * E
    total, budget = a["x"].astype(np.float64) + b["x"].astype(np.float64), 0.0
    for step in (1, 2):
        m1, ph, m2, dq = ([torch.empty(E * m, device=DEV) for _ in range(2)] for m in (L.msg1_len, plan.p_total, L.msg2_len, L.msg2_len))
        for i in (0, 1):
            plan.project(X[i], Q[i], m1[i])
        for i in (0, 1):
            plan.orthogonalize(m1[i], m1[1 - i], ph[i], mask[i])
            plan.backproject(X[i], ph[i], m2[i])
        for i in (0, 1):
            plan.diff(m2[i], m2[1 - i], Q[i], dq[i], mask[i])
            plan.apply(X[i], ph[i], dq[i], m1[1 - i], w, mask[i])
        assert torch.equal(ph[0], ph[1]) and torch.equal(dq[0], dq[1]) and torch.equal(Q[0], Q[1]), step
        xa, xb = (t.cpu().numpy() for t in X)
        budget = budget + 2.0 * np.spacing(np.maximum(np.abs(xa), np.abs(xb)))  # 2 ulp per element per step
        assert np.all(np.abs(xa.astype(np.float64) + xb - total) <= budget), step
    assert not torch.equal(Q[0], flat(a["q"]))


@pytest.mark.parametrize("r,E", [(4, 4), (2, 7), (8, 2)])
def test_fused_step_vs_loop(r, E):
    from chocosgd_amd import codec, powergossip
    L, rng = PO.Layout(RESNET20ISH, r), np.random.RandomState(E)
    info = {j: 1.0 / (E + 1) for j in range(E + 1)}  # worker 1: the high end of edge (0, 1), the low end of the others
    runs = [(powergossip.fused_step, DEV, torch.float32), (powergossip.step_loop, "cpu", torch.float64),
            (powergossip.step_loop, "cpu", torch.float32)]
    models = [model(RESNET20ISH, d, dt) for _, d, dt in runs]
    comps = [powergossip.PowerGossipCompressor(r, Peers(7), info, seed=1) for _ in runs]
    for step in range(2):  # the second step reads the warm Q and the momentum buffers
        grads = spread(rng, L.n)
        for (fn, _, _), (ps, groups, names, state), comp in zip(runs, models, comps):
            set_grads(ps, L, grads)
            c0 = codec.launch_count("lowrank_gossip_apply_mfma_kernel")
            assert fn(comp, groups, names, state) == 32 * E * (L.msg1_len + L.msg2_len)
            assert codec.launch_count("lowrank_gossip_apply_mfma_kernel") - c0 == (fn is powergossip.fused_step)
        for name, get in (("params", lambda i: cat(models[i][0])), ("Q", lambda i: cat([comps[i].q]))):
            d, dist = np.abs(get(2) - get(1)).max(), np.abs(get(0) - get(1)).max()
            print(f"wide r={r} E={E} step {step} {name}: d = {d:.3g}, fused distance {dist:.3g}")
            assert dist <= 4 * d, (name, step)
