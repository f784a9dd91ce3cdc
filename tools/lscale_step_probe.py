"""Cost of dynamic loss scaling in front of the batched SGD update on master weights.

    python tools/lscale_step_probe.py [--out FILE] [--steps 50] [--warmup 5] [--reps 5]
                                      [--only-existing] [--root DIR]

One JSON line: ResNet-50's 161 tensors / 25.6 M elements in fp16 with fp32 master weights (each
parameter its own allocation; momentum 0.9, weight decay 1e-4, max_norm 0.25), three things timed
in ONE process, interleaved window by window:
  (a) torch_*   what a user has with torch.amp.GradScaler in front of the step: its unscale_ op
                (torch._amp_foreach_non_finite_check_and_unscale_), torch.nn.utils.clip_grad_norm_,
                the found_inf.item() branch, utils.apply_gradient(master=) and
                torch._amp_update_scale_ -- the yardstick.  Timed TWICE per round (a1 before, a2
                after the others): |a1 - a2| is the run-to-run spread a difference has to beat
  (b) scaled_*  utils.apply_gradient(master=, clip_norm=, loss_scale=)
  (c) clip_*    today's utils.apply_gradient(master=, clip_norm=)
  host_us       host wall time per step: `steps` steps queued, one synchronise, divided
  gpu_us        the same window between two device events
  kernel_us_*   dispatch-attached time per step, profiling in a window of its own: the three
                kernels of (b); param_sgd_master_gclip_kernel in (c); param_sgd_kernel in a plain
                fp32 utils.apply_gradient(flat_out=)
(medians over `reps` rounds after `warmup` steps of each).  The scale is 1 and never grows, so
that (a)'s in-place unscale leaves the gradients as they are from step to step.
--only-existing: (c) and the two existing kernels alone, for a tree that does not have loss
scaling; --root DIR imports the package from that tree (the parent's checkout, built).
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
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
from chocosgd_amd import codec, utils  # noqa: E402

DEV = "cuda"
HP = {"lr": 0.1, "weight_decay": 1e-4, "momentum": 0.9, "dampening": 0.0, "nesterov": False}
MAX_NORM = 0.25  # --rnn_clip's default


def layout():
    with open(os.path.join(ROOT, "tests", "golden", "layouts.json")) as f:
        return json.load(f)["resnet50_imagenet"]


def model(lens, dtype, master, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(m, generator=g, device=DEV).to(dtype)) for m in lens]
    for p in params:
        p.grad = (0.01 * torch.randn(p.shape, generator=g, device=DEV)).to(dtype)
    groups = [dict(HP, params=[p], name=f"p{i}") for i, p in enumerate(params)]
    mw = utils.MasterWeights(groups, list(enumerate(gr["name"] for gr in groups))) if master else None
    return params, groups, collections.defaultdict(dict), mw


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


def measure(lens, steps, warmup, reps, only_existing):
    pc, gc, sc, mc = model(lens, torch.float16, True)
    pf, gf, sf, _ = model(lens, torch.float32, False)
    flat = torch.empty(sum(lens), dtype=torch.float32, device=DEV)

    def clip_step():
        utils.apply_gradient(gc, sc, master=mc, clip_norm=MAX_NORM)

    def plain_fp32_step():
        utils.apply_gradient(gf, sf, flat_out=flat)

    order = [("clip", clip_step)]
    if not only_existing:
        pa, ga, sa, ma = model(lens, torch.float16, True)
        pb, gb, sb, mb = model(lens, torch.float16, True)
        scaler = utils.LossScaler(DEV, init_scale=1.0, growth_interval=2 ** 30)
        t_scale = torch.ones(1, device=DEV)
        t_tracker = torch.zeros(1, dtype=torch.int32, device=DEV)
        t_found = torch.zeros(1, device=DEV)
        grads_a = [p.grad for p in pa]

        def torch_step():
            t_found.zero_()
            torch._amp_foreach_non_finite_check_and_unscale_(grads_a, t_found, t_scale.double().reciprocal().float())
            torch.nn.utils.clip_grad_norm_(pa, MAX_NORM)
            if t_found.item() == 0.0:
                utils.apply_gradient(ga, sa, master=ma)
            torch._amp_update_scale_(t_scale, t_tracker, t_found, 2.0, 0.5, 2 ** 30)

        def scaled_step():
            utils.apply_gradient(gb, sb, master=mb, clip_norm=MAX_NORM, loss_scale=scaler)

        order = [("torch1", torch_step), ("scaled", scaled_step), ("clip", clip_step), ("torch2", torch_step)]
    for _, fn in order:
        window(fn, warmup)
    runs = collections.defaultdict(list)
    for _ in range(reps):
        for key, fn in order:
            runs[key].append(window(fn, steps))
    row = {"layout": "resnet50_fp16_master", "tensors": len(lens), "elements": sum(lens), "steps": steps,
           "warmup": warmup, "reps": reps, "max_norm": MAX_NORM, "tree": "parent" if only_existing else "this"}
    for key in runs:
        row[f"{key}_host_us"] = round(statistics.median(r[0] for r in runs[key]), 1)
        row[f"{key}_gpu_us"] = round(statistics.median(r[1] for r in runs[key]), 1)
        row[f"{key}_gpu_us_min_max"] = [round(min(r[1] for r in runs[key]), 1), round(max(r[1] for r in runs[key]), 1)]
    if not only_existing:
        row["spread_gpu_us"] = round(abs(row["torch1_gpu_us"] - row["torch2_gpu_us"]), 1)
        row["spread_host_us"] = round(abs(row["torch1_host_us"] - row["torch2_host_us"]), 1)
        row["scaled_minus_clip_gpu_us"] = round(row["scaled_gpu_us"] - row["clip_gpu_us"], 1)
        row["scaled_minus_clip_host_us"] = round(row["scaled_host_us"] - row["clip_host_us"], 1)
        best = min(row["torch1_gpu_us"], row["torch2_gpu_us"])
        row["scaled_over_torch_gpu"] = round(row["scaled_gpu_us"] / best, 3)
        row["scaled_over_torch_host"] = round(row["scaled_host_us"] / min(row["torch1_host_us"], row["torch2_host_us"]), 3)
        kt = kernel_times(scaled_step, ["param_sqnorm_kernel", "param_gradnorm_scaled_total_kernel",
                                        "param_sgd_master_scaled_kernel"], steps)
        for nm, (us, cnt) in kt.items():
            short = nm.replace("param_", "").replace("_kernel", "")
            row[f"kernel_us_{short}"], row[f"kernel_launches_{short}"] = us, cnt
    us, cnt = kernel_times(clip_step, ["param_sgd_master_gclip_kernel"], steps)["param_sgd_master_gclip_kernel"]
    row["kernel_us_sgd_master_gclip"], row["kernel_launches_sgd_master_gclip"] = us, cnt
    window(plain_fp32_step, warmup)
    us, cnt = kernel_times(plain_fp32_step, ["param_sgd_kernel"], steps)["param_sgd_kernel"]
    row["kernel_us_sgd"], row["kernel_launches_sgd"] = us, cnt
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-existing", action="store_true")
    ap.add_argument("--root")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    assert args.steps >= 20 and args.warmup >= 5, "at least 20 timed steps after 5 warm-ups"
    row = measure(layout(), args.steps, args.warmup, args.reps, args.only_existing)
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
