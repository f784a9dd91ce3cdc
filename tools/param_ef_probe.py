"""Cost of a whole DeepSqueeze step and a whole EF-signSGD step (deep_squeeze.py:94-127,
ef_sign_sgd.py:78-123) with and without the error-feedback kernels.

    python tools/param_ef_probe.py [--out FILE] [--steps 50] [--reps 5]

One JSON line per layout (ResNet-50 in fp32 and in bf16; each parameter its own allocation;
weight decay + momentum; the sign compressor; 3 ranks whose exchange is replayed -- every
neighbour's message is this rank's own):
  ds_loop_*, ef_loop_*     deep_squeeze.step_loop / ef_sign.step_loop: the op sequence that ran
                           before the kernels (batched apply_gradient, pack, one torch op per
                           dense line, unpack)
  ds_fused_*, ef_fused_*   deep_squeeze.fused_step / ef_sign.fused_step
  host_us       host wall time per step: `steps` steps queued, one synchronise, divided
  gpu_us        the same window between two device events
  launches      device activities (kernels + copies) of one step, from torch.profiler
(medians over `reps` windows after a warm-up window; the loop's and the fused step's windows
alternate, in one process), and for each new kernel, launched alone:
  kernel_us_*, kernel_tbps_*   dispatch-attached time of param_ef_kernel in each of its three
                uses (accum, apply, apply | div | scale) and of sign_local_residual (in place
                with no local copy: DeepSqueeze; in place with the local copy: EF-signSGD), and
                the bytes each moves divided by it
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
from chocosgd_amd import codec, deep_squeeze, ef_sign  # noqa: E402
from chocosgd_amd.wire import _Layout  # noqa: E402
from chocosgd_amd.tensor_buffer import TensorBuffer  # noqa: E402

DEV = P.DEV
W, RANK = 3, 1
INFO = {r: 1.0 / W for r in range(W)}


class Replay:
    """In the aggregators' place: every rank's message is this rank's own."""

    def _agg(self, data, op=None, force_wait=True, communication_scheme=None, async_op=False):
        every = [data] * W
        return every if communication_scheme == "all_gather" else dict(enumerate(every))


def ds_step(which, lens, dtype):
    params, groups, names = P.model(lens, dtype)
    state = collections.defaultdict(dict)
    shapes = [(p.size(), p.nelement()) for p in params]
    memory = TensorBuffer.from_flat(torch.zeros(sum(lens), device=DEV), [p.size() for p in params])
    comp = deep_squeeze.DeepSqueezeCompressor(aggregator=Replay(), rank=RANK, comm_op="sign", comm_device="gpu",
                                              compress_ratio=0.9, quantize_level=4, is_biased=False, backend="nccl",
                                              use_ipc=False, consensus_stepsize=0.5)
    fn = getattr(deep_squeeze, which)
    return lambda: fn(comp, groups, names, state, shapes, memory, INFO)


def ef_step(which, lens, dtype):
    params, groups, names = P.model(lens, dtype)
    state = collections.defaultdict(dict)
    memory = TensorBuffer.from_flat(torch.zeros(sum(lens), device=DEV), [p.size() for p in params])
    comp = ef_sign.EFSignCompressor(rank=RANK, world_size=W, aggregator=Replay(), comm_op="sign", comm_device="gpu",
                                    use_ipc=False)
    fn = getattr(ef_sign, which)
    return lambda: fn(comp, groups, names, state, memory)


def alternate(a, b, iters, reps):
    """Medians of (host_us, gpu_us) of a and of b over windows that alternate a, b, a, b, ..."""
    for fn in (a, b):
        P.events(fn, max(2, iters // 10))  # warm-up: code objects, the allocator's blocks, first-step buffers
    ra, rb = [], []
    for _ in range(reps):
        ra.append(P.events(a, iters))
        rb.append(P.events(b, iters))
    med = lambda runs: (statistics.median(r[0] for r in runs), statistics.median(r[1] for r in runs))  # noqa: E731
    return med(ra), med(rb)


def kernels(lens, dtype):
    """Each new kernel launched alone: {tag: (kernel name, bytes, fn)}."""
    n, esz = sum(lens), torch.empty(0, dtype=dtype).element_size()
    params, _, _ = P.model(lens, dtype)
    plan = codec.ParamSgdPlan(params)
    for i, p in enumerate(params):
        plan.param_ptrs[i] = p.data_ptr()
    flat, local = torch.zeros(n, device=DEV), torch.empty(n, device=DEV)
    lay = _Layout.get(tuple(lens), torch.device(DEV, torch.cuda.current_device()))
    norms = torch.ones(len(lens), device=DEV)
    resid = lambda lo: codec.sign_local_residual(flat, norms, seg_off=lay.seg_off, nseg=lay.nseg, local_out=lo,  # noqa: E731
                                                 resid_out=flat)
    return {
        "ef_accum": ("param_ef_kernel", n * (esz + 8), lambda: plan.ef(flat, codec.EF_ACCUM)),
        "ef_apply": ("param_ef_kernel", n * (2 * esz + 4), lambda: plan.ef(flat, codec.EF_APPLY)),
        "ef_apply_div_scale": ("param_ef_kernel", n * (2 * esz + 8),
                               lambda: plan.ef(flat, codec.EF_APPLY | codec.EF_DIV | codec.EF_SCALE, lr=0.1, divisor=3.0)),
        "residual": ("sign_local_residual", n * 8, lambda: resid(None)),
        "residual_local": ("sign_local_residual", n * 12, lambda: resid(local)),
    }


def measure(name, lens, dtype, steps, reps):
    row = {"layout": name, "tensors": len(lens), "elements": sum(lens), "param_dtype": str(dtype).split(".")[-1],
           "compressor": "sign", "ranks": W, "steps": steps, "reps": reps}
    for tag, make in (("ds", ds_step), ("ef", ef_step)):
        loop, fused = make("step_loop", lens, dtype), make("fused_step", lens, dtype)
        (lh, lg), (fh, fg) = alternate(loop, fused, steps, reps)
        row.update({f"{tag}_loop_host_us": round(lh, 1), f"{tag}_loop_gpu_us": round(lg, 1),
                    f"{tag}_loop_launches": P.count_launches(loop),
                    f"{tag}_fused_host_us": round(fh, 1), f"{tag}_fused_gpu_us": round(fg, 1),
                    f"{tag}_fused_launches": P.count_launches(fused)})
    for tag, (kernel, nbytes, fn) in kernels(lens, dtype).items():
        t, launches = P.kernel_time(fn, kernel)
        row[f"bytes_{tag}"] = nbytes
        if t:
            row.update({f"kernel_us_{tag}": round(t, 2), f"kernel_launches_{tag}": launches,
                        f"kernel_tbps_{tag}": round(nbytes / t / 1e6, 3)})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    rows = []
    for name, lens, dtype in P.layouts():
        if not name.startswith("resnet50"):
            continue
        rows.append(measure(name, lens, dtype, args.steps, args.reps))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
