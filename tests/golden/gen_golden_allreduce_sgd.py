"""Golden-vector generator for the centralized branch of SGD.step
(dl_code/pcode/optim/sgd.py:68-92), plain all-reduce data-parallel SGD.

Runs ONLY in the authoring container, where the upstream reference is mounted read-only at
/root/reference: it runs the reference's own SGD.step on CPU fp32 tensors as rank 0 of a world
of 3 -- comm.get_data, TensorBuffer, CentralizedAggregation._agg(op="avg") and
optim.utils.apply_gradient are the reference's -- and records inputs and outputs as .npz
fixtures next to this script.  Nothing from the reference is copied: the fixtures are data only.

The optimizer and its aggregator are made with object.__new__ (their constructors want a
process group and the training configuration) and given the attributes the step reads
(group=None, world_size=3.0).  `dist` in the reference's communication module is replaced by a
stand-in whose all_reduce adds the two peers' recorded gradients in place, peer 1 then peer 2.

    sgd_inputs.npz (gen_golden_sgd.py's)   lens, p0 and rank 0's gradients g0, g1, g2
    allreduce_sgd_peers.npz                the peers' gradients q1_<k>, q2_<k> (flat)
    allreduce_sgd_sums.npz                 world = 3.0, and per step k: sum<k> (the buffer after
                                           the all-reduce) and avg<k> (what _agg returns); they
                                           do not depend on the hyperparameters, which the
                                           generator asserts, and are stored once
    allreduce_sgd_<set>.npz                hp = [lr, weight_decay, momentum, dampening,
                                           nesterov], and after each of three consecutive steps
                                           k: p<k>, buf<k> (momentum sets) -- all flat

The peers' gradients hold special values against rank 0's ordinary ones, the other way round
and against each other, sums that are subnormal, a normal sum whose third is subnormal, and
inf + -inf.  Every step gets fresh gradient tensors (the reference rebinds p.grad to the
momentum buffer).

Usage:  python tests/golden/gen_golden_allreduce_sgd.py
"""
import collections
import contextlib
import os
import sys
import types

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference

import numpy as np  # noqa: E402
import torch  # noqa: E402

REF = "/root/reference/dl_code"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, OUT)
# the reference's sparsification module imports the unvendored bit2byte packing extension, which
# nothing here calls: an empty module lets the import pass (gen_golden.py stubs it the same way)
sys.modules.setdefault("bit2byte", types.ModuleType("bit2byte"))

import pcode.optim.sgd as ref_sgd  # noqa: E402
import pcode.utils.communication as ref_comm  # noqa: E402
from gen_golden_sgd import SETS, STEPS  # noqa: E402

WORLD = 3.0


def peers(lens, gs):
    rng = np.random.RandomState(20240911)
    n = sum(lens)
    qs = [[(rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n)).astype(np.float32) for _ in range(STEPS)]
          for _ in range(2)]
    sub = np.float32(1e-41)
    special = [0.0, -0.0, np.inf, -np.inf, np.nan, sub, -sub, 1e-38]
    base = lens[0] + lens[1] + 100  # gen_golden_sgd.py: rank 0's specials sit at base + 20 + i and base + 40 + i
    for k in range(STEPS):
        q1, q2 = qs[0][k], qs[1][k]
        for i, v in enumerate(special):
            q1[base + 200 + i] = v                                # a peer's special against ordinary values
            q2[base + 220 + i] = special[(i + k) % len(special)]
            q1[base + 240 + i], q2[base + 240 + i] = v, special[(i + k + 3) % len(special)]  # against each other
            q1[base + 40 + i] = special[(i + 2 * k + 2) % len(special)]  # against rank 0's specials
        # inf + -inf at rank 0's +inf and -inf
        q1[base + 20 + 2], q2[base + 20 + 2] = -np.inf, 1.0
        q1[base + 20 + 3], q2[base + 20 + 3] = 2.0, np.inf
        # subnormal sums at rank 0's subnormals; 1e-38 + 0 + 0, whose third is subnormal
        q1[base + 20 + 5], q2[base + 20 + 5] = 3e-41, -2e-42
        q1[base + 20 + 6], q2[base + 20 + 6] = 1e-41, 1e-45
        q1[base + 20 + 7], q2[base + 20 + 7] = 0.0, -0.0
        # ordinary values cancelling to a subnormal and to zero
        g = gs[k]
        q1[base + 300], q2[base + 300] = -g[base + 300], 7e-42
        q1[base + 301], q2[base + 301] = -g[base + 301], 0.0
    return qs


def split(flat, lens):
    out, o = [], 0
    for m in lens:
        out.append(torch.from_numpy(flat[o:o + m].copy()))
        o += m
    return out


def cat(tensors):
    return np.concatenate([t.detach().numpy().reshape(-1) for t in tensors]).astype(np.float32)


def run(hp, lens, p0, gs, qs):
    lr, wd, mom, damp, nest = hp
    params = [torch.nn.Parameter(t) for t in split(p0, lens)]
    groups = [{"params": [p], "name": f"p{i}", "param_size": p.size(), "nelement": p.nelement(), "lr": lr,
               "weight_decay": wd, "momentum": mom, "dampening": damp, "nesterov": nest}
              for i, p in enumerate(params)]
    rec = {}
    step = [0]

    def all_reduce(data, op=None, group=None, async_op=False):
        assert op == "SUM" and group is None and not async_op
        data.add_(torch.from_numpy(qs[0][step[0]])).add_(torch.from_numpy(qs[1][step[0]]))
        rec[f"sum{step[0]}"] = data.detach().numpy().copy()

    ref_comm.dist = types.SimpleNamespace(all_reduce=all_reduce, ReduceOp=types.SimpleNamespace(SUM="SUM"))
    agg = object.__new__(ref_comm.CentralizedAggregation)
    agg.rank, agg.group, agg.world_size = 0, None, WORLD
    ref_agg = agg._agg

    def recording_agg(*args, **kwargs):
        out = ref_agg(*args, **kwargs)
        rec[f"avg{step[0]}"] = out.detach().numpy().copy()
        return out

    agg._agg = recording_agg
    opt = object.__new__(ref_sgd.SGD)
    opt.param_groups, opt.state = groups, collections.defaultdict(dict)
    opt.param_names = list(enumerate(g["name"] for g in groups))
    opt.world_aggregator = agg
    opt.conf = types.SimpleNamespace(is_centralized=True, epoch_=0, distributed=True)
    out = {"hp": np.array([lr, wd, mom, damp, float(nest)], dtype=np.float64)}
    for k in range(STEPS):
        step[0] = k
        for p, g in zip(params, split(gs[k], lens)):
            p.grad = g
        n_bits = opt.step(timer=lambda *a, **kw: contextlib.nullcontext())
        assert n_bits == 32 * sum(lens)
        out[f"p{k}"] = cat([p.data for p in params])
        if mom != 0:
            out[f"buf{k}"] = cat([opt.state[p]["momentum_buffer"] for p in params])
    return out, rec


def main():
    inputs = np.load(os.path.join(OUT, "sgd_inputs.npz"))
    lens, p0 = inputs["lens"].tolist(), inputs["p0"]
    gs = [inputs[f"g{k}"] for k in range(STEPS)]
    qs = peers(lens, gs)
    path = os.path.join(OUT, "allreduce_sgd_peers.npz")
    np.savez_compressed(path, **{f"q{r + 1}_{k}": qs[r][k] for r in range(2) for k in range(STEPS)})
    print(path, os.path.getsize(path))
    sums = None
    for name, hp in SETS.items():
        out, rec = run(hp, lens, p0, gs, qs)
        if sums is None:
            sums = rec
        assert sums.keys() == rec.keys() and all(
            np.array_equal(sums[key].view(np.uint32), rec[key].view(np.uint32)) for key in rec)
        path = os.path.join(OUT, f"allreduce_sgd_{name}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path))
    path = os.path.join(OUT, "allreduce_sgd_sums.npz")
    np.savez_compressed(path, world=np.float64(WORLD), **sums)
    print(path, os.path.getsize(path))
    for k in range(STEPS):
        s, a = sums[f"sum{k}"], sums[f"avg{k}"]
        with np.errstate(all="ignore"):
            sub = np.isfinite(s) & (s != 0) & (np.abs(s) < np.float32(1.17549435e-38))
            recip = (s * np.float32(1.0 / 3.0)).astype(np.float32)
        differ = np.isfinite(a) & (recip.view(np.uint32) != a.view(np.uint32))
        print(f"step {k}: nan sums {int(np.isnan(s).sum())}, subnormal sums {int(sub.sum())}, "
              f"a reciprocal multiply differs on {int(differ.sum())} of {s.size}")


if __name__ == "__main__":
    main()
