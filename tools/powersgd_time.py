"""Time of the PowerSGD kernels (csrc/lowrank.hip, csrc/lowrank_mfma.hip) and of the whole step, against the plain
all-reduce SGD step on the same layout in the same process and against each stage's compulsory
bytes at 8 TB/s.

    python tools/powersgd_time.py [--out profiles/powersgd_time.json] [--iters 20] [--warmup 5] [--reps 5] [--ranks 8,16]
                                  [--orth {mgs,cholqr}]

One JSON line per rank of codec.LOWRANK_RANKS (or --ranks) on ResNet-50's layout (161 tensors, 25,557,032 fp32 elements,
each parameter its own allocation; the shapes are written out below and checked against
tests/golden/layouts.json), with a loopback aggregator (the all-reduces return their buffer):
  step_us / allreduce_us   device time per call of powersgd.fused_step and of
             utils.allreduce_sgd_step between two events (`iters` calls a window after `warmup`,
             the two alternating window by window; the median over `reps` windows, min and max)
  kernel_us_*    the dispatch-attached time of each kernel's launches alone (the library's
             profile hooks), in a window of its own; ranks 8, 16 and 32 run the *_mfma_kernel
             of a stage and are reported under the stage's one name
  bytes_* / floor_us_* / tbps_*   the stage's compulsory traffic (project: 12 B per compressed
             element, read g and e, write M; back-project: 4 B; decode: 12 B, read M, write the
             sum and e; the uncompressed tensors' copy: 8 B per element in project and decode),
             the time it takes at 8 TB/s, and the rate the kernel reached
  --orth cholqr  the step orthogonalises by Cholesky-QR (csrc/lowrank_cholqr.hip; ranks 8, 16 and 32): its three
             launches are timed one by one and summed as kernel_us_cholqr, and the modified Gram-Schmidt step of a
             second compressor on a model of its own runs in the same process, its windows alternating with the
             others: step_mgs_us and kernel_us_mgs (lowrank_orth_kernel in that step)
  msg_elements   what is sent (message 1 + message 2) against the layout's elements
Needs a ROCm device; there is no fall-back.
"""
import argparse
import collections
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import param_sgd_probe as P  # noqa: E402
from chocosgd_amd import codec, powersgd, utils  # noqa: E402

PEAK_TBPS = 8.0
STAGES = {"lowrank_project_kernel": 12, "lowrank_backproject_kernel": 4, "lowrank_decode_kernel": 12}
OTHERS = ["lowrank_orth_kernel", "lowrank_slabsum_kernel", "param_pack_kernel", "param_sgd_flatgrad_kernel"]
CHOLQR = ["lowrank_gram_kernel", "lowrank_chol_kernel", "lowrank_orthapply_kernel"]


def resnet50_shapes():
    """torchvision's resnet50 parameters in state order (bottleneck blocks, v1.5 strides do not change shapes)."""
    s, inplanes = [(64, 3, 7, 7), (64,), (64,)], 64
    for planes, blocks in ((64, 3), (128, 4), (256, 6), (512, 3)):
        for b in range(blocks):
            s += [(planes, inplanes, 1, 1), (planes,), (planes,), (planes, planes, 3, 3), (planes,), (planes,),
                  (4 * planes, planes, 1, 1), (4 * planes,), (4 * planes,)]
            if b == 0:
                s += [(4 * planes, inplanes, 1, 1), (4 * planes,), (4 * planes,)]
            inplanes = 4 * planes
    return s + [(1000, 2048), (1000,)]


def measure(shapes, r, iters, warmup, reps, orth="mgs"):
    agg = P._Loopback()
    _, ga, na = P.model(shapes, torch.float32)
    _, gb, nb = P.model(shapes, torch.float32)
    sa, sb = collections.defaultdict(dict), collections.defaultdict(dict)
    comp = powersgd.PowerSGDCompressor(r, agg, orthogonalize=orth)
    ways = {"step": lambda: powersgd.fused_step(comp, ga, na, sa),
            "allreduce": lambda: utils.allreduce_sgd_step(gb, nb, sb, agg)}
    if orth == "cholqr":  # the parent's method beside it, window by window
        _, gc, nc = P.model(shapes, torch.float32)
        sc, comp_mgs = collections.defaultdict(dict), powersgd.PowerSGDCompressor(r, agg)
        ways["step_mgs"] = lambda: powersgd.fused_step(comp_mgs, gc, nc, sc)
    for fn in ways.values():
        P.events(fn, warmup)
    plan = comp.plan
    n_comp = sum(m for m, c in zip(plan.lens, plan.compressed) if c)
    row = {"layout": "resnet50_fp32", "rank": r, "orth": orth, "tensors": len(shapes), "elements": plan.n,
           "compressed_tensors": sum(plan.compressed), "compressed_elements": n_comp,
           "msg_elements": plan.msg1_len + plan.msg2_len, "iters": iters, "warmup": warmup, "reps": reps}
    runs = {tag: [] for tag in ways}
    for _ in range(reps):
        for tag, fn in ways.items():
            runs[tag].append(P.events(fn, iters)[1])
    for tag in ways:
        row[f"{tag}_us"] = round(statistics.median(runs[tag]), 1)
        row[f"{tag}_us_min_max"] = [round(min(runs[tag]), 1), round(max(runs[tag]), 1)]
    row["step_vs_allreduce"] = round(row["step_us"] / row["allreduce_us"], 2)
    total = 0.0
    for kernel in list(STAGES) + OTHERS + (CHOLQR if orth == "cholqr" else []):
        t, launches = P.kernel_time(ways["step"], kernel, iters)
        if not t and kernel in STAGES:  # the matrix-instruction kernel of the stage
            t, launches = P.kernel_time(ways["step"], kernel.replace("_kernel", "_mfma_kernel"), iters)
        if not t:
            continue
        total += t
        row[f"kernel_us_{kernel}"], row[f"kernel_launches_{kernel}"] = round(t, 2), launches
        if kernel in STAGES:
            nbytes = STAGES[kernel] * n_comp + (0 if kernel == "lowrank_backproject_kernel" else 8 * (plan.n - n_comp))
            row[f"bytes_{kernel}"], row[f"floor_us_{kernel}"] = nbytes, round(nbytes / PEAK_TBPS / 1e6, 2)
            row[f"tbps_{kernel}"] = round(nbytes / t / 1e6, 3)
    row["kernel_us_step"] = round(total, 2)
    if orth == "cholqr":
        row["kernel_us_cholqr"] = round(sum(row[f"kernel_us_{k}"] for k in CHOLQR), 2)
        row["kernel_us_mgs"] = round(P.kernel_time(ways["step_mgs"], "lowrank_orth_kernel", iters)[0], 2)
        row["cholqr_vs_mgs"] = round(row["kernel_us_cholqr"] / row["kernel_us_mgs"], 3)
    t, _ = P.kernel_time(ways["allreduce"], "param_sgd_flatgrad_kernel", iters)
    t2, _ = P.kernel_time(ways["allreduce"], "param_pack_kernel", iters)
    if t and t2:
        row["kernel_us_allreduce"] = round(t + t2, 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "powersgd_time.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ranks", default=",".join(str(r) for r in codec.LOWRANK_RANKS))
    ap.add_argument("--orth", choices=codec.LOWRANK_ORTH_METHODS, default="mgs")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the timer needs a ROCm device"
    shapes = resnet50_shapes()
    with open(os.path.join(ROOT, "tests", "golden", "layouts.json")) as f:
        assert [int(torch.Size(s).numel()) for s in shapes] == json.load(f)["resnet50_imagenet"]
    rows = []
    for r in (int(x) for x in args.ranks.split(",")):
        rows.append(measure(shapes, r, args.iters, args.warmup, args.reps, args.orth))
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
