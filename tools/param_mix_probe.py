"""Cost of the dense half of a DCD-PSGD step in front of its compressor (dcd_psgd.py:96-125),
with and without the neighbour-mix kernel.

    python tools/param_mix_probe.py [--out FILE] [--steps 100] [--reps 5]

One JSON line per layout (ResNet-50 in fp32 and in bf16, 3000 tensors of 100 elements; each
parameter its own allocation; weight decay + momentum; a ring's M = 3 replicas, weights 1/3):
  (a) torch_*   what runs without the kernel: the batched apply_gradient(apply_grad_to_model=
                False), the two packs (params, grads) and the reference's expression
                sum([hat * w ...]) - lr * grads, one torch op per term
  (b) mix_*     the batched apply_gradient and ONE params_mix call (GRAD_SUB, flat_out = the half
                params, x_out = the packed params), as dcd.fused_step runs them
  host_us       host wall time per step: `steps` steps queued, one synchronise, divided
  gpu_us        the same window between two device events
  launches      device activities (kernels + copies) of one step, from torch.profiler
  kernel_us_*, kernel_tbps_*   dispatch-attached time of param_mix_kernel and, in the same run,
                of param_sgd_kernel (the yardstick: same tile shape, a comparable stream count),
                and the bytes each moves divided by it
(medians over `reps` windows after a warm-up window).  Both variants run in one process.
"""
import argparse
import collections
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import param_sgd_probe as P  # noqa: E402
from chocosgd_amd import codec, utils  # noqa: E402
from chocosgd_amd.tensor_buffer import TensorBuffer  # noqa: E402

DEV = P.DEV
INFO = {0: 1.0 / 3, 1: 1.0 / 3, 2: 1.0 / 3}


def replicas(params):
    g = torch.Generator(device=DEV).manual_seed(7)
    flat = torch.cat([p.detach().float().reshape(-1) for p in params])
    sizes = [p.size() for p in params]
    return {r: TensorBuffer.from_flat(flat + 0.01 * torch.randn(flat.shape, generator=g, device=DEV), sizes)
            for r in INFO}


def measure(name, lens, dtype, steps, reps):
    n, esz = sum(lens), torch.empty(0, dtype=dtype).element_size()
    pa, ga, na = P.model(lens, dtype)
    sa, ha = collections.defaultdict(dict), replicas(pa)
    lr = ga[0]["lr"]

    def torch_step():
        utils.apply_gradient(ga, sa, apply_grad_to_model=False)
        TensorBuffer([p.data for p in pa], dtype=torch.float32)
        grads = TensorBuffer([p.grad.data for p in pa], dtype=torch.float32)
        return utils.weighted_sum([h.buffer for h in ha.values()], list(INFO.values())) - lr * grads.buffer

    pb, gb, nb = P.model(lens, dtype)
    sb, hb = collections.defaultdict(dict), replicas(pb)
    entries = utils.step_entries(gb, nb, "param_mix_probe", need_grads=True)

    def mix_step():
        plan = utils.grad_step_plan(entries, sb, hb)
        half, packed = (torch.empty(n, dtype=torch.float32, device=DEV) for _ in range(2))
        plan.mix([h.buffer for h in hb.values()], list(INFO.values()), lr=lr, mode=codec.MIX_GRAD_SUB, flat_out=half,
                 x_out=packed)
        return half

    torch_host, torch_gpu = P.median_of(torch_step, steps, reps)
    mix_host, mix_gpu = P.median_of(mix_step, steps, reps)
    mix_bytes = n * (len(INFO) * 4 + 2 * esz + 8)   # reads M replicas, g, p; writes half and packed
    sgd_bytes = n * 5 * esz                         # grad mode: reads p, g, buf; writes buf, g
    k_mix, l_mix = P.kernel_time(mix_step, "param_mix_kernel")
    k_sgd, l_sgd = P.kernel_time(mix_step, "param_sgd_kernel")
    row = {"layout": name, "tensors": len(lens), "elements": n, "param_dtype": str(dtype).split(".")[-1],
           "sources": len(INFO), "steps": steps, "reps": reps,
           "torch_host_us": round(torch_host, 1), "torch_gpu_us": round(torch_gpu, 1),
           "torch_launches": P.count_launches(torch_step),
           "mix_host_us": round(mix_host, 1), "mix_gpu_us": round(mix_gpu, 1), "mix_launches": P.count_launches(mix_step),
           "mix_bytes": mix_bytes, "sgd_bytes": sgd_bytes}
    if k_mix:
        row.update(kernel_us_mix=round(k_mix, 2), kernel_launches_mix=l_mix,
                   kernel_tbps_mix=round(mix_bytes / k_mix / 1e6, 3))
    if k_sgd:
        row.update(kernel_us_sgd=round(k_sgd, 2), kernel_launches_sgd=l_sgd,
                   kernel_tbps_sgd=round(sgd_bytes / k_sgd / 1e6, 3))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    rows = []
    for name, lens, dtype in P.layouts():
        rows.append(measure(name, lens, dtype, args.steps, args.reps))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
