"""Cholesky-QR orthogonalisation on the device (csrc/lowrank_cholqr.hip) on test_gpu_powersgd_highrank.py's layout:
P of 12 (r = 8: under a tile), 33, 257 (one over a block), 300 and 2049 rows (nine blocks)."""
import numpy as np
import pytest
import torch

import _cholqr_oracle as CO
import _powersgd_oracle as PO
import _streams as ST
from conftest import same_bits
from test_gpu_powersgd_highrank import DEV, RANKS, SHAPES, Loopback, cat, dev, model, set_grads, spread

pytestmark = pytest.mark.gpu
KERNELS = ["lowrank_gram_kernel", "lowrank_chol_kernel", "lowrank_orthapply_kernel", "lowrank_orth_kernel"]


def message(L, r, kind="gaussian"):
    rng = np.random.RandomState(r)  # Gaussian message 1, or per matrix U diag(logspace(0, -3, r)) V^T: condition number 1e3
    x = rng.standard_normal(L.msg1_len).astype(np.float32)
    for _, ps, _, rows, _ in L.matrices() if kind == "graded" else ():
        U, V = (np.linalg.qr(rng.standard_normal((n, r)))[0] for n in (rows, r))
        x[ps] = ((U * np.logspace(0, -3, r)) @ V.T).reshape(-1)
    return x


def run(plan, x):
    msg1 = dev(x)
    plan.orthogonalize(msg1, "cholqr")
    return msg1.cpu().numpy()


@pytest.mark.parametrize("kind", ["gaussian", "graded"])
@pytest.mark.parametrize("r", RANKS)
def test_orthogonalize(r, kind):
    """Against fp64 Gram-Schmidt at lowrank_orth_kernel's allowance (4 d, d the fp32 restatement's distance; the fp64
    Cholesky-QR rounded once stood at 0.07 to 0.17 of d Gaussian, 0.55 to 0.91 graded, on the CPU), and against the
    contract's oracle within half an fp32 ulp of the element plus 4 x the oracle's own spread between ascending and
    descending Gram blocks (measured on the CPU: 1.4e-17 Gaussian, 4.2e-13 / 4.5e-13 / 6.4e-13 graded at r = 8 / 16 / 32)."""
    from chocosgd_amd import codec
    plan, L = codec.LowRankPlan(SHAPES, r, DEV), PO.Layout(SHAPES, r)
    x = message(L, r, kind)
    got, d, dist, noise, excess = run(plan, x), 0.0, 0.0, 0.0, -1.0
    for _, ps, _, rows, _ in L.matrices():
        P, G = x[ps].reshape(rows, r), got[ps].reshape(rows, r).astype(np.float64)
        want, ora = PO.orthogonalize(P), CO.orthogonalize(P)
        d = max(d, np.abs(PO.orthogonalize(P, np.float32) - want).max())
        dist = max(dist, np.abs(G - want).max())
        noise = max(noise, np.abs(CO.orthogonalize(P, order=-1) - ora).max())
        excess = max(excess, (np.abs(G - ora) - np.spacing(np.abs(ora).astype(np.float32)) / 2).max())
    print(f"cholqr r={r} {kind}: d = {d:.3g}, kernel distance {dist:.3g}; oracle: half an ulp + {excess:.3g}, spread {noise:.3g}")
    assert dist <= 4 * d and excess <= 4 * noise
    assert same_bits(run(plan, x), got), "the same bits twice"
    assert all(same_bits(got[t], x[t]) for _, t in L.tails()), "the tail is not touched"
    # a zero matrix, a zero last column, an exactly duplicated column (held to finite and zero only)
    ps = [m[1] for m in L.matrices()]
    x[ps[0]] = 0.0
    x[ps[1]].reshape(-1, r)[:, r - 1] = 0.0
    x[ps[2]].reshape(-1, r)[:, 3] = x[ps[2]].reshape(-1, r)[:, 1]
    got = run(plan, x)
    assert np.isfinite(got).all() and not got[ps[0]].any() and not got[ps[1]].reshape(-1, r)[:, r - 1].any()
    assert not got[ps[2]].reshape(-1, r)[:, 3].any() and got[ps[2]].reshape(-1, r)[:, 4].any()


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("r", RANKS)
def test_fused_step_vs_loop(r, world):
    from chocosgd_amd import codec, powersgd
    L, rng = PO.Layout(SHAPES, r), np.random.RandomState(world)
    runs = [(powersgd.fused_step, DEV, torch.float32), (powersgd.step_loop, "cpu", torch.float64), (powersgd.step_loop, "cpu", torch.float32)]
    models = [model(SHAPES, d, dt) for _, d, dt in runs]
    comps = [powersgd.PowerSGDCompressor(r, Loopback(world, 7), seed=1, orthogonalize="cholqr") for _ in runs]
    for step in range(2):  # the second step reads e, the warm Q and the momentum buffers
        flat = spread(rng, L.n)
        for (fn, _, _), (ps, groups, names, state), comp in zip(runs, models, comps):
            set_grads(ps, L, flat)
            c0 = [codec.launch_count(k) for k in KERNELS]
            assert fn(comp, groups, names, state) == 32 * (L.msg1_len + L.msg2_len)
            assert [codec.launch_count(k) - c for k, c in zip(KERNELS, c0)] == ([1, 1, 1, 0] if fn is powersgd.fused_step else [0] * 4)
        for name, get in (("params", lambda i: cat(models[i][0])), ("e", lambda i: cat([comps[i].e])), ("Q", lambda i: cat([comps[i].q]))):
            d, dist = np.abs(get(2) - get(1)).max(), np.abs(get(0) - get(1)).max()
            print(f"cholqr r={r} W={world} step {step} {name}: d = {d:.3g}, fused distance {dist:.3g}")
            assert dist <= 4 * d, (name, step)


def test_streams():
    from chocosgd_amd import codec
    plan, L = codec.LowRankPlan(SHAPES, 16, DEV), PO.Layout(SHAPES, 16)
    true = {"msg1": dev(message(L, 16))}
    work, poison = {"msg1": true["msg1"].clone()}, {"msg1": true["msg1"] * 0.5 + 1.0}
    plan.orthogonalize(work["msg1"], "cholqr")  # on the null stream, from the true input: the bits expected on the side stream
    want = work["msg1"].clone()
    got = ST.run(lambda: plan.orthogonalize(work["msg1"], "cholqr"), work, true, poison, family="powersgd", case="orthogonalize_cholqr")
    assert torch.equal(got[1]["msg1"], want)
