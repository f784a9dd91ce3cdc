"""Cost of one consensus evaluation (--evaluate_consensus, distributed_running_cv.py:110-115,
:239-243) with auxiliary.consensus_eval against the torch sequence it replaces.

    python tools/consensus_time.py [--out FILE] [--iters 200] [--reps 5]

One JSON line per layout (ResNet-50 and ResNet-20, in fp32 and in bf16; each parameter its own
allocation).  No collective is timed: the aggregator hands the packed buffer back as the "sum" and
keeps world_size = 3, so that both sides divide by 3 and measure the same distance, ||x / 3 - x||:
  torch_*       the reference's sequence on the same machine in the same process: deepcopy of
                the model, per-tensor division by the world size (what agg_model's _agg leaves
                when the all-reduce is taken out), per-tensor subtraction, cat, norm and .item()
  eval_*        auxiliary.consensus_eval(model, agg) -- the distance alone, no copy of the model
                -- ended, like the torch sequence, by reading the distance on the host
  eval_avg_*    auxiliary.consensus_eval(model, agg, avg_out=copy): the averaged model as well
  host_us       host wall time per call: `iters` calls, one synchronise at the end, divided
  gpu_us        the same window between two device events
  launches      device activities (kernels + copies) of one call, from torch.profiler
(medians over `reps` windows after a warm-up window; the three alternate, in one process), the
algorithmic bytes of each and, launched alone, the dispatch-attached time
of param_consensus_kernel in its three modes and of param_consensus_total_kernel.
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import param_sgd_probe as P  # noqa: E402
from chocosgd_amd import auxiliary, codec  # noqa: E402

DEV = P.DEV
WORLD = 3.0


class Alone:
    """world 3, no collective: _agg hands the buffer back."""
    world_size = WORLD

    def _agg(self, data, op=None, distributed=True):
        return data


class Model(torch.nn.Module):
    def __init__(self, lens, dtype, seed):
        super().__init__()
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.ps = torch.nn.ParameterList(
            [torch.nn.Parameter(torch.randn(m, generator=g, device=DEV).to(dtype)) for m in lens])


def torch_sequence(model):
    """deepcopy, agg_model's division per tensor, get_model_difference's lines."""
    copied = copy.deepcopy(model)
    for param in copied.parameters():
        param.data = param.data / WORLD
    diffs = [w2 - w1 for w1, w2 in zip(model.parameters(), copied.parameters())]
    return torch.cat([d.clone().detach().view(-1) for d in diffs]).norm().item()


def layouts():
    with open(os.path.join(ROOT, "tests", "golden", "layouts.json")) as f:
        table = json.load(f)
    return [(f"{short}_{tag}", table[name], dtype)
            for short, name in (("resnet50", "resnet50_imagenet"), ("resnet20", "resnet20_cifar10"))
            for tag, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16))]


def kernels(model, n):
    """Each mode of the new kernels launched alone: {tag: (kernel name, bytes, fn)}."""
    params = list(model.parameters())
    esz = params[0].element_size()
    plan = codec.ParamSgdPlan(params)
    for i, p in enumerate(params):
        plan.param_ptrs[i] = p.data_ptr()
    xsum = torch.randn(n, device=DEV)
    out = [torch.empty_like(p.data) for p in params]
    return {
        "dist": ("param_consensus_kernel", n * (4 + esz), lambda: plan.consensus(xsum, WORLD)),
        "dist_write": ("param_consensus_kernel", n * (4 + 2 * esz), lambda: plan.consensus(xsum, WORLD, avg_out=out)),
        "write": ("param_consensus_kernel", n * (4 + esz), lambda: plan.consensus(xsum, WORLD, avg_out=out,
                                                                                  want_dist=False)),
        "total": ("param_consensus_total_kernel", 0, lambda: plan.consensus(xsum, WORLD)),
    }


def measure(name, lens, dtype, iters, reps):
    n, esz = sum(lens), torch.empty(0, dtype=dtype).element_size()
    model, avg = Model(lens, dtype, 0), Model(lens, dtype, 1)
    agg = Alone()
    fns = {
        "torch": lambda: torch_sequence(model),
        "eval": lambda: auxiliary.consensus_eval(model, agg)[0][0].item(),
        "eval_avg": lambda: auxiliary.consensus_eval(model, agg, avg_out=avg)[0][0].item(),
    }
    row = {"layout": name, "tensors": len(lens), "elements": n, "param_dtype": str(dtype).split(".")[-1],
           "iters": iters, "reps": reps,
           # deepcopy r+w, division r+w, subtraction 2r+w, cat r+w (fp32 result of a 16-bit difference stays
           # 16-bit in torch: every pass moves esz), norm r
           "bytes_torch": n * esz * 10,
           # the pack esz r + 4 w, the kernel 4 + esz r (+ esz w)
           "bytes_eval": n * (8 + 2 * esz), "bytes_eval_avg": n * (8 + 3 * esz)}
    for fn in fns.values():
        P.events(fn, max(2, iters // 10))  # warm-up: code objects, the allocator's blocks, the plan's workspace
    runs = {tag: [] for tag in fns}
    for _ in range(reps):
        for tag, fn in fns.items():
            runs[tag].append(P.events(fn, iters))
    for tag, fn in fns.items():
        row[f"{tag}_host_us"] = round(statistics.median(r[0] for r in runs[tag]), 1)
        row[f"{tag}_gpu_us"] = round(statistics.median(r[1] for r in runs[tag]), 1)
        row[f"{tag}_launches"] = P.count_launches(fn)
    row["speedup_eval"] = round(row["torch_gpu_us"] / row["eval_gpu_us"], 2)
    row["speedup_eval_avg"] = round(row["torch_gpu_us"] / row["eval_avg_gpu_us"], 2)
    # same inputs, both ways: the fp32 norm of the torch sequence against the fp64-accumulated one
    row["distance_torch"], row["distance_eval"] = fns["torch"](), fns["eval"]()
    for tag, (kernel, nbytes, fn) in kernels(model, n).items():
        t, launches = P.kernel_time(fn, kernel)
        if t:
            row.update({f"kernel_us_{tag}": round(t, 2), f"kernel_launches_{tag}": launches})
            if nbytes:
                row.update({f"bytes_{tag}": nbytes, f"kernel_tbps_{tag}": round(nbytes / t / 1e6, 3)})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the timer needs a ROCm device"
    rows = []
    for name, lens, dtype in layouts():
        rows.append(measure(name, lens, dtype, args.iters, args.reps))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
