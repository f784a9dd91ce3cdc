"""PowerSGD at ranks 8, 16 and 32 on the device (csrc/lowrank_mfma.hip): test_gpu_powersgd.py's checks and
helpers on a layout of its own.  The kernels stage 256 columns of Q, slabs and orthogonalise's stage are 256
rows, a tile is 16 rows: SHAPES has 257 and 2049 in either dimension, a 12-row matrix (r = 8 only), rows off
the 16 grid, odd cols, the aligned path ((33, 1100), (2049, 40)), cols = 4 mod 16, 4-D, the rule's edge at r = 32."""
import numpy as np
import pytest
import torch

import _powersgd_oracle as PO
import _streams as ST
from conftest import same_bits
from test_gpu_powersgd import DEV, SENTINEL, Loopback, cat, dev, model, set_grads, setup, spread

pytestmark = pytest.mark.gpu
RANKS = [8, 16, 32]
SHAPES = [(7,), (40, 2049), (), (64, 257), (0,), (33, 1100), (12, 100), (2049, 40), (5, 5), (257, 68), (100, 36, 3, 3),
          (300, 9)]
KERNELS = ["lowrank_project_mfma_kernel", "lowrank_orth_kernel", "lowrank_backproject_mfma_kernel",
           "lowrank_slabsum_kernel", "lowrank_decode_mfma_kernel", "lowrank_project_kernel",
           "lowrank_backproject_kernel", "lowrank_decode_kernel"]


def ratio(got, A, B, terms):
    """max |got - A B| / ((terms + 2) 2^-24 |A| |B|): at most 1 for a length-`terms` fp32 dot product in any order."""
    A, B = A.astype(np.float64), B.astype(np.float64)
    bound = (terms + 2) * 2.0 ** -24 * (np.abs(A) @ np.abs(B))
    return float((np.abs(got - A @ B) / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("r", RANKS)
def test_project(r):
    plan, L, a = setup(r, SHAPES)
    runs = []
    for _ in range(2):
        e, msg1 = dev(a["e"]), torch.full((L.msg1_len,), SENTINEL, device=DEV)
        plan.project(dev(a["g"]), e, dev(a["q"]), msg1)
        runs.append((e.cpu().numpy(), msg1.cpu().numpy()))
    (e, msg1), M, worst = runs[0], a["e"].copy(), 0.0
    for f, ps, qs, rows, cols in L.matrices():
        M[f] = a["g"][f] + a["e"][f]
        worst = max(worst, ratio(msg1[ps].reshape(rows, r), M[f].reshape(rows, cols), a["q"][qs].reshape(cols, r), cols))
    print(f"project r={r}: worst error / bound = {worst:.3g}")
    assert worst <= 1.0
    assert same_bits(e, M), "M over e; the uncompressed tensors' e untouched"
    assert all(same_bits(msg1[t], a["g"][f]) for f, t in L.tails())
    assert same_bits(runs[1][0], e) and same_bits(runs[1][1], msg1), "the same bits twice"


@pytest.mark.parametrize("r", RANKS)
def test_backproject(r):
    plan, L, a = setup(r, SHAPES, seed=10)
    runs = []
    for _ in range(2):
        msg2 = torch.full((L.msg2_len,), SENTINEL, device=DEV)
        plan.backproject(dev(a["e"]), dev(a["msg1"]), msg2)
        runs.append(msg2.cpu().numpy())
    worst = max(ratio(runs[0][qs].reshape(cols, r), a["e"][f].reshape(rows, cols).T, a["msg1"][ps].reshape(rows, r), rows)
                for f, ps, qs, rows, cols in L.matrices())
    print(f"back-project r={r}: worst error / bound = {worst:.3g}")
    assert worst <= 1.0
    assert same_bits(runs[0], runs[1])


@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("r", RANKS)
def test_decode(r, W):
    plan, L, a = setup(r, SHAPES, seed=20)
    for f, _ in L.tails():
        a["e"][f] = SENTINEL
    runs = []
    for _ in range(2):
        e, out = dev(a["e"]), torch.full((L.n,), SENTINEL, device=DEV)
        plan.decode(e, dev(a["msg1"]), dev(a["msg2"]), out, float(W))
        runs.append((e.cpu().numpy(), out.cpu().numpy()))
    (e, out), want_e, worst = runs[0], a["e"].copy(), 0.0
    for f, ps, qs, rows, cols in L.matrices():
        worst = max(worst, ratio(out[f].reshape(rows, cols), a["msg1"][ps].reshape(rows, r), a["msg2"][qs].reshape(cols, r).T, r - 1))
        want_e[f] = a["e"][f] - out[f] / np.float32(W)
    print(f"decode r={r} W={W}: worst error / bound = {worst:.3g}")
    assert worst <= 1.0
    assert same_bits(e, want_e), "e = fl(M - fl(out / W)) from the out the kernel wrote; sentinels untouched"
    assert all(same_bits(out[f], a["msg1"][t]) for f, t in L.tails())
    assert same_bits(runs[1][0], e) and same_bits(runs[1][1], out), "the same bits twice"


@pytest.mark.parametrize("r", RANKS)
def test_orthogonalize(r):
    from chocosgd_amd import codec
    plan, L = codec.LowRankPlan(SHAPES, r, DEV), PO.Layout(SHAPES, r)
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
    tail = min(t.start for _, t in L.tails())
    assert same_bits(got[tail:], x[tail:]), "the tail is not touched"
    # a zero matrix, and a zero last column among Gaussian ones: finite, zeros stay zeros
    ps = [m[1] for m in L.matrices()]
    x[ps[0]] = 0.0
    x[ps[1]].reshape(-1, r)[:, r - 1] = 0.0
    msg1 = dev(x)
    plan.orthogonalize(msg1)
    got = msg1.cpu().numpy()
    assert np.isfinite(got).all() and not got[ps[0]].any() and not got[ps[1]].reshape(-1, r)[:, r - 1].any()


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("r", RANKS)
def test_fused_step_vs_loop(r, world):
    from chocosgd_amd import codec, powersgd
    L, rng = PO.Layout(SHAPES, r), np.random.RandomState(world)
    runs = [(powersgd.fused_step, DEV, torch.float32), (powersgd.step_loop, "cpu", torch.float64),
            (powersgd.step_loop, "cpu", torch.float32)]
    models = [model(SHAPES, d, dt) for _, d, dt in runs]
    comps = [powersgd.PowerSGDCompressor(r, Loopback(world, 7), seed=1) for _ in runs]
    launches = [1, 1, 1, 1, 1, 0, 0, 0]  # 257 and 2049 rows: the slab sum runs; the vector kernels do not
    for step in range(2):  # the second step reads e, the warm Q and the momentum buffers
        flat = spread(rng, L.n)
        for (fn, _, _), (ps, groups, names, state), comp in zip(runs, models, comps):
            set_grads(ps, L, flat)
            c0 = [codec.launch_count(k) for k in KERNELS]
            assert fn(comp, groups, names, state) == 32 * (L.msg1_len + L.msg2_len)
            assert [codec.launch_count(k) - c for k, c in zip(KERNELS, c0)] == (launches if fn is powersgd.fused_step else [0] * 8)
        for name, get in (("params", lambda i: cat(models[i][0])), ("e", lambda i: cat([comps[i].e])),
                          ("Q", lambda i: cat([comps[i].q]))):
            d, dist = np.abs(get(2) - get(1)).max(), np.abs(get(0) - get(1)).max()
            print(f"r={r} W={world} step {step} {name}: d = {d:.3g}, fused distance {dist:.3g}")
            assert dist <= 4 * d, (name, step)


@pytest.mark.parametrize("call", ["project", "orthogonalize", "backproject", "decode"])
def test_streams(call):
    plan, L, a = setup(16, SHAPES)
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
