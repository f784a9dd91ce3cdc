"""Golden-vector generator for the consensus evaluation of the reference
(dl_code/pcode/distributed_running_cv.py:110-115, :239-243): agg_model(copy, op="avg")
(pcode/utils/communication.py:114-122) and get_model_difference(model, copy)
(pcode/utils/auxiliary.py:18-34).

Runs ONLY in the authoring container, where the upstream reference is mounted read-only at
/root/reference: it runs the reference's own agg_model and get_model_difference on CPU fp32
tensors as rank 0 of a world of 3 and records inputs and outputs as .npz fixtures next to this
script.  Nothing from the reference is copied: the fixtures are data only.

The aggregator is made with object.__new__ (its constructor wants a process group) and given
the attributes the calls read (group=None, world_size=3.0).  `dist` in the reference's
communication module is replaced by a stand-in whose all_reduce adds the two peers' recorded
tensors in place, peer 1 then peer 2.  The layout is sgd_inputs.npz's `lens`.

    consensus_<set>.npz   lens, world = 3.0, x0 / x1 / x2 (the three workers' flat models), sum
                          (every tensor after its all-reduce, flat), avg (the copy after
                          agg_model, flat), distance (the reference's get_model_difference(model,
                          copy), a Python float stored as fp64) and distance64 (sqrt of the exactly
                          summed squares of the recorded fp32 avg - x0)
    set "ordinary":       ordinary values, a finite distance; also ref_rel_gap =
                          |distance - distance64| / distance64, the error of the reference's fp32
                          norm, asserted to lie within n * 2^-24
    set "special":        special values placed as gen_golden_allreduce_sgd.py places them: rank 0's
                          against ordinary ones, the peers' against ordinary ones, against rank 0's
                          and against each other, subnormal sums, a normal sum whose third is
                          subnormal, inf + -inf, NaN, +-0

Usage:  python tests/golden/gen_golden_consensus.py
"""
import copy
import math
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

import pcode.utils.auxiliary as ref_aux  # noqa: E402
import pcode.utils.communication as ref_comm  # noqa: E402

WORLD = 3.0


def workers(lens, special):
    rng = np.random.RandomState(20241020)
    n = sum(lens)
    x0, x1, x2 = ((rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n)).astype(np.float32) for _ in range(3))
    if not special:
        return x0, x1, x2
    sub = np.float32(1e-41)
    sp = [0.0, -0.0, np.inf, -np.inf, np.nan, sub, -sub, 1e-38]
    base = lens[0] + lens[1] + 100
    for i, v in enumerate(sp):
        x0[base + 20 + i] = v                             # rank 0's special against what the peers hold there
        x0[base + 40 + i] = sp[(i + 5) % len(sp)]
        x1[base + 200 + i] = v                            # a peer's special against ordinary values
        x2[base + 220 + i] = sp[(i + 1) % len(sp)]
        x1[base + 240 + i], x2[base + 240 + i] = v, sp[(i + 3) % len(sp)]  # against each other
        x1[base + 40 + i] = sp[(i + 2) % len(sp)]         # against rank 0's specials
    # inf + -inf at rank 0's +inf and -inf
    x1[base + 20 + 2], x2[base + 20 + 2] = -np.inf, 1.0
    x1[base + 20 + 3], x2[base + 20 + 3] = 2.0, np.inf
    # subnormal sums at rank 0's subnormals; 1e-38 + 0 + 0, whose third is subnormal
    x1[base + 20 + 5], x2[base + 20 + 5] = 3e-41, -2e-42
    x1[base + 20 + 6], x2[base + 20 + 6] = 1e-41, 1e-45
    x1[base + 20 + 7], x2[base + 20 + 7] = 0.0, -0.0
    # ordinary values cancelling to a subnormal and to zero
    x1[base + 300], x2[base + 300] = -x0[base + 300], 7e-42
    x1[base + 301], x2[base + 301] = -x0[base + 301], 0.0
    # a normal sum whose third is subnormal (1e-38 is itself below the smallest normal fp32)
    x0[base + 302], x1[base + 302], x2[base + 302] = 2e-38, 0.0, -0.0
    x0[base + 303], x1[base + 303], x2[base + 303] = 1e-38, 1e-38, 1e-38
    # a sum of -0 (every worker holds -0) next to the +0 sums above
    x0[base + 304], x1[base + 304], x2[base + 304] = -0.0, -0.0, -0.0
    return x0, x1, x2


class Model(torch.nn.Module):
    def __init__(self, flat, lens):
        super().__init__()
        offs = np.concatenate([[0], np.cumsum(lens)])
        self.ps = torch.nn.ParameterList(
            [torch.nn.Parameter(torch.from_numpy(flat[offs[s]:offs[s + 1]].copy())) for s in range(len(lens))])


def cat(model):
    return np.concatenate([p.detach().numpy().reshape(-1) for p in model.parameters()]).astype(np.float32)


def run(lens, xs):
    offs = np.concatenate([[0], np.cumsum(lens)])
    model = Model(xs[0], lens)
    sums, call = [], [0]

    def all_reduce(data, op=None, group=None, async_op=False):
        assert op == "SUM" and group is None and not async_op
        s = call[0]
        call[0] += 1
        assert data.numel() == lens[s]
        data.add_(torch.from_numpy(xs[1][offs[s]:offs[s + 1]])).add_(torch.from_numpy(xs[2][offs[s]:offs[s + 1]]))
        sums.append(data.detach().numpy().copy())

    ref_comm.dist = types.SimpleNamespace(all_reduce=all_reduce, ReduceOp=types.SimpleNamespace(SUM="SUM"))
    agg = object.__new__(ref_comm.CentralizedAggregation)
    agg.rank, agg.group, agg.world_size = 0, None, WORLD
    copied = copy.deepcopy(model)
    agg.agg_model(copied, "avg")
    assert call[0] == len(lens)
    distance = ref_aux.get_model_difference(model, copied)
    assert np.array_equal(cat(model).view(np.uint32), xs[0].view(np.uint32)), "the model itself is untouched"
    return np.concatenate(sums).astype(np.float32), cat(copied), float(distance)


def main():
    lens = np.load(os.path.join(OUT, "sgd_inputs.npz"))["lens"].tolist()
    n = sum(lens)
    for name, special in (("ordinary", False), ("special", True)):
        xs = workers(lens, special)
        s, a, distance = run(lens, xs)
        with np.errstate(all="ignore"):
            d = (a - xs[0]).astype(np.float32)
            finite = bool(np.isfinite(d).all())
            distance64 = math.sqrt(math.fsum((d.astype(np.float64) ** 2).tolist())) if finite else float(
                np.sqrt(np.sum(d.astype(np.float64) ** 2)))
        out = {"lens": np.array(lens, dtype=np.int64), "world": np.float64(WORLD), "x0": xs[0], "x1": xs[1],
               "x2": xs[2], "sum": s, "avg": a, "distance": np.float64(distance), "distance64": np.float64(distance64)}
        if not special:
            assert finite and math.isfinite(distance) and distance64 > 0
            gap = abs(distance - distance64) / distance64
            assert gap <= n * 2.0 ** -24, gap  # the worst case of an fp32 accumulation over n squares
            out["ref_rel_gap"] = np.float64(gap)
            print(f"{name}: distance {distance!r}, distance64 {distance64!r}, ref_rel_gap {gap:.3e}")
        else:
            assert not math.isfinite(distance) and not math.isfinite(distance64)
            with np.errstate(all="ignore"):
                sub = np.isfinite(s) & (s != 0) & (np.abs(s) < np.float32(1.17549435e-38))
                recip = (s * np.float32(1.0 / 3.0)).astype(np.float32)
            differ = np.isfinite(a) & (recip.view(np.uint32) != a.view(np.uint32))
            print(f"{name}: distance {distance!r}; nan sums {int(np.isnan(s).sum())}, subnormal sums {int(sub.sum())}, "
                  f"a reciprocal multiply differs on {int(differ.sum())} of {s.size}")
        path = os.path.join(OUT, f"consensus_{name}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
