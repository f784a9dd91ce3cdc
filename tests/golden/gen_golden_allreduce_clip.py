"""Golden-vector generator for the language-model loop's step with the centralized optimizer:
torch.nn.utils.clip_grad_norm_(model.parameters(), conf.rnn_clip) on the local gradients
(dl_code/pcode/distributed_running_nlp.py:96) followed by the centralized branch of SGD.step
(dl_code/pcode/optim/sgd.py:68-92).

Runs ONLY in the authoring container, where the upstream reference is mounted read-only at
/root/reference: it runs torch's own clip and the reference's own SGD.step on CPU fp32 tensors
as rank 0 of a world of 3, exactly as gen_golden_allreduce_sgd.py builds the optimizer and its
aggregator, and records inputs and outputs as .npz fixtures next to this script.  The two peers
clip their own gradients by their own norms (the same torch call) before the stand-in
all_reduce adds them, peer 1 then peer 2.  Nothing from the reference is copied: the fixtures
are data only.

    allreduce_clip_inputs.npz   lens, p0, max_norm, world, and per step k: g<k> (rank 0's raw
                                gradients), total0_<k>, total1_<k>, total2_<k> (what
                                clip_grad_norm_ returned on each rank), c1_<k>, c2_<k> (the
                                peers' CLIPPED gradients), sum<k> (the buffer after the
                                all-reduce), avg<k> (what _agg returned) -- all flat
    allreduce_clip_<set>.npz    hp = [lr, weight_decay, momentum, dampening, nesterov], and after
                                each of three consecutive steps k: p<k>, buf<k> (momentum sets)

Layout: a zero-length tensor, 8195 crosses a tile with cut groups at both ends.  The gradient
scale falls from step to step so that, with the one max_norm, every rank's step 0 is clipped
(c < 1) and step 2 is not (c == 1).

Usage:  python tests/golden/gen_golden_allreduce_clip.py
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
# the reference's sparsification module imports the unvendored bit2byte packing extension, which
# nothing here calls: an empty module lets the import pass (gen_golden.py stubs it the same way)
sys.modules.setdefault("bit2byte", types.ModuleType("bit2byte"))

import pcode.optim.sgd as ref_sgd  # noqa: E402
import pcode.utils.communication as ref_comm  # noqa: E402

LENS = [5, 1, 0, 8195, 33, 300, 17]
STEPS = 3
WORLD = 3.0
MAX_NORM = 0.4                      # exps/finetune-lstm/example.sh
STEP_SCALE = [1.0, 0.01, 1e-4]
SETS = {  # lr, weight_decay, momentum, dampening, nesterov
    "clip": (0.1, 0.0, 0.0, 0.0, False),
    "nesterov": (0.1, 5e-4, 0.9, 0.0, True),
    "damp": (0.01, 1e-4, 0.9, 0.1, False),
}


def split(flat):
    out, o = [], 0
    for m in LENS:
        out.append(torch.from_numpy(flat[o:o + m].copy()))
        o += m
    return out


def cat(tensors):
    return np.concatenate([t.detach().numpy().reshape(-1) for t in tensors]).astype(np.float32)


def inputs():
    """p0, and the three ranks' raw gradients per step."""
    rng = np.random.RandomState(20241103)
    n = sum(LENS)
    p0 = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32)
    raw = [[(rng.standard_normal(n) * STEP_SCALE[k] * (1.0 + 0.5 * r)).astype(np.float32) for k in range(STEPS)]
           for r in range(3)]
    for k in range(STEPS):
        raw[0][k][7], raw[0][k][8] = 0.0, -0.0
    return p0, raw


def clipped(flat):
    """torch's clip on one rank's gradients: (the total it returned, the clipped gradients)."""
    ps = [torch.nn.Parameter(torch.zeros(m)) for m in LENS]
    for p, g in zip(ps, split(flat)):
        p.grad = g
    total = torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
    return total.numpy().astype(np.float32).reshape(()), cat([p.grad for p in ps])


def run(hp, p0, raw, peers):
    lr, wd, mom, damp, nest = hp
    params = [torch.nn.Parameter(t) for t in split(p0)]
    groups = [{"params": [p], "name": f"p{i}", "param_size": p.size(), "nelement": p.nelement(), "lr": lr,
               "weight_decay": wd, "momentum": mom, "dampening": damp, "nesterov": nest}
              for i, p in enumerate(params)]
    rec = {}
    step = [0]

    def all_reduce(data, op=None, group=None, async_op=False):
        assert op == "SUM" and group is None and not async_op
        data.add_(torch.from_numpy(peers[0][step[0]])).add_(torch.from_numpy(peers[1][step[0]]))
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
        for p, g in zip(params, split(raw[k])):
            p.grad = g
        total = torch.nn.utils.clip_grad_norm_(params, MAX_NORM)  # distributed_running_nlp.py:96
        rec[f"total0_{k}"] = total.numpy().astype(np.float32).reshape(())
        n_bits = opt.step(timer=lambda *a, **kw: contextlib.nullcontext())
        assert n_bits == 32 * sum(LENS)
        out[f"p{k}"] = cat([p.data for p in params])
        if mom != 0:
            out[f"buf{k}"] = cat([opt.state[p]["momentum_buffer"] for p in params])
    return out, rec


def main():
    torch.set_num_threads(1)
    p0, raw = inputs()
    peers, totals = [[], []], {}
    for r in (1, 2):
        for k in range(STEPS):
            totals[f"total{r}_{k}"], c = clipped(raw[r][k])
            peers[r - 1].append(c)
    common = None
    for name, hp in SETS.items():
        out, rec = run(hp, p0, raw[0], peers)
        if common is None:
            common = rec
        assert common.keys() == rec.keys() and all(
            np.array_equal(common[key].view(np.uint32), rec[key].view(np.uint32)) for key in rec)
        path = os.path.join(OUT, f"allreduce_clip_{name}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path))
    totals.update({k: v for k, v in common.items() if k.startswith("total")})
    for r in range(3):  # what the tests rely on: step 0 is clipped on every rank, step 2 on none
        assert float(totals[f"total{r}_0"]) > 10 * MAX_NORM and float(totals[f"total{r}_2"]) < 0.1 * MAX_NORM
    path = os.path.join(OUT, "allreduce_clip_inputs.npz")
    np.savez_compressed(path, lens=np.array(LENS, dtype=np.int64), p0=p0, max_norm=np.float64(MAX_NORM),
                        world=np.float64(WORLD), **totals,
                        **{f"g{k}": raw[0][k] for k in range(STEPS)},
                        **{f"c{r}_{k}": peers[r - 1][k] for r in (1, 2) for k in range(STEPS)},
                        **{k: v for k, v in common.items() if not k.startswith("total")})
    print(path, os.path.getsize(path), {k: float(v) for k, v in sorted(totals.items())})


if __name__ == "__main__":
    main()
