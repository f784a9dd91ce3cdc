"""Cost of global-norm gradient clipping in front of the batched SGD update.

    python tools/gclip_step_probe.py [--out FILE] [--steps 50] [--warmup 5] [--reps 5] [--only-plain]

One JSON line per layout (ResNet-50, 161 tensors / 25.6 M elements, in fp32 and in bf16; each
parameter its own allocation; momentum 0.9, weight decay 1e-4, apply mode with flat_out), three
things timed in ONE process, interleaved window by window:
  (a) torch_*   torch.nn.utils.clip_grad_norm_(params, max_norm) followed by utils.apply_gradient:
                what a user has without the fused path, the yardstick.  Timed TWICE per round
                (a1 before, a2 after the others): |a1 - a2| is the run-to-run spread a difference
                has to beat
  (b) fused_*   utils.apply_gradient(clip_norm=max_norm)
  (c) plain_*   utils.apply_gradient alone (no clipping)
  host_us       host wall time per step: `steps` steps queued, one synchronise, divided
  gpu_us        the same window between two device events
  kernel_us_*   dispatch-attached time per step, profiling in a window of its own:
                param_sqnorm_kernel, param_gradnorm_total_kernel and param_sgd_gclip_kernel in (b),
                param_sgd_kernel in (c)
(medians over `reps` rounds after `warmup` steps of each).  --only-plain: (c) alone, for a library
that does not have the clipped entry points (CHOCO_CODEC_LIB: the parent's build).
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chocosgd_amd import codec, utils  # noqa: E402

DEV = "cuda"
HP = {"lr": 0.1, "weight_decay": 1e-4, "momentum": 0.9, "dampening": 0.0, "nesterov": False}
MAX_NORM = 0.25  # --rnn_clip's default


def layouts():
    with open(os.path.join(ROOT, "tests", "golden", "layouts.json")) as f:
        r50 = json.load(f)["resnet50_imagenet"]
    return [("resnet50_fp32", r50, torch.float32), ("resnet50_bf16", r50, torch.bfloat16)]


def model(lens, dtype, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(m, generator=g, device=DEV).to(dtype)) for m in lens]
    for p in params:
        p.grad = (0.01 * torch.randn(p.shape, generator=g, device=DEV)).to(dtype)
    groups = [dict(HP, params=[p], name=f"p{i}") for i, p in enumerate(params)]
    flat = torch.empty(sum(lens), dtype=torch.float32, device=DEV)
    return params, groups, collections.defaultdict(dict), flat


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6, a.elapsed_time(b) / iters * 1e3


def kernel_times(fn, names, iters):
    """Dispatch-attached time of each kernel of `names` per call of fn (us, launches)."""
    codec.profile_reset()
    codec.profile_filter(list(names))
    codec.profile_enable(True)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    codec.profile_enable(False)
    out = {}
    for nm in names:
        t, c = codec.profile_read(nm)
        out[nm] = (round(t / iters * 1e3, 2), c // iters) if c else (None, 0)
    codec.profile_filter(None)
    codec.profile_reset()
    return out


def measure(name, lens, dtype, steps, warmup, reps, only_plain):
    pa, ga, sa, fa = model(lens, dtype)
    pb, gb, sb, fb = model(lens, dtype)
    pc, gc, sc, fc = model(lens, dtype)

    def torch_step():
        torch.nn.utils.clip_grad_norm_(pa, MAX_NORM)
        utils.apply_gradient(ga, sa, flat_out=fa)

    def fused_step():
        utils.apply_gradient(gb, sb, flat_out=fb, clip_norm=MAX_NORM)

    def plain_step():
        utils.apply_gradient(gc, sc, flat_out=fc)

    order = [("plain", plain_step)] if only_plain else \
        [("torch1", torch_step), ("fused", fused_step), ("plain", plain_step), ("torch2", torch_step)]
    for _, fn in order:
        window(fn, warmup)
    runs = collections.defaultdict(list)
    for _ in range(reps):
        for key, fn in order:
            runs[key].append(window(fn, steps))
    row = {"layout": name, "tensors": len(lens), "elements": sum(lens), "param_dtype": str(dtype).split(".")[-1],
           "steps": steps, "warmup": warmup, "reps": reps, "max_norm": MAX_NORM,
           "lib": os.path.basename(os.environ.get("CHOCO_CODEC_LIB") or "product")}
    for key in runs:
        row[f"{key}_host_us"] = round(statistics.median(r[0] for r in runs[key]), 1)
        row[f"{key}_gpu_us"] = round(statistics.median(r[1] for r in runs[key]), 1)
        row[f"{key}_gpu_us_min_max"] = [round(min(r[1] for r in runs[key]), 1), round(max(r[1] for r in runs[key]), 1)]
    if not only_plain:
        row["spread_gpu_us"] = round(abs(row["torch1_gpu_us"] - row["torch2_gpu_us"]), 1)
        row["spread_host_us"] = round(abs(row["torch1_host_us"] - row["torch2_host_us"]), 1)
        row["gain_gpu_us"] = round(min(row["torch1_gpu_us"], row["torch2_gpu_us"]) - row["fused_gpu_us"], 1)
        row["gain_host_us"] = round(min(row["torch1_host_us"], row["torch2_host_us"]) - row["fused_host_us"], 1)
        kt = kernel_times(fused_step, ["param_sqnorm_kernel", "param_gradnorm_total_kernel", "param_sgd_gclip_kernel"],
                          steps)
        for nm, (us, cnt) in kt.items():
            short = nm.replace("param_", "").replace("_kernel", "")
            row[f"kernel_us_{short}"], row[f"kernel_launches_{short}"] = us, cnt
    us, cnt = kernel_times(plain_step, ["param_sgd_kernel"], steps)["param_sgd_kernel"]
    row["kernel_us_sgd"], row["kernel_launches_sgd"] = us, cnt
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-plain", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert args.steps >= 20 and args.warmup >= 5, "at least 20 timed steps after 5 warm-ups"
    rows = []
    for name, lens, dtype in layouts():
        rows.append(measure(name, lens, dtype, args.steps, args.warmup, args.reps, args.only_plain))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
