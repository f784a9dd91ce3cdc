"""Cost of DGC's optimizer half with clipping and momentum-factor masking on, up to the point
where the message is ready (sync, recover_info and the unpack are the same in both).

    python tools/dgc_step_probe.py [--out FILE] [--steps 100] [--reps 5] [--norm-ab] [--no-steps]

One JSON line per layout (ResNet-50 in fp32 and in bf16, 3000 tensors of 100 elements; each
parameter its own allocation; weight decay, momentum, clip and mask all on, top-k at 0.99):
  (a) loop_*    what runs without the batched kernels: DGC._apply_gradient's per-tensor loop with
                _clip_gradient (dgc.py:254-324, written out below with torch alone; its
                `grad_norm >= threshold` reads a device scalar per tensor, as the reference's
                does), then DGCCodec.compress as it was (flatten, add_, the segmented top-k, the
                sparse clear of the memory) and a per-tensor masking loop over the selection
  (b) fused_*   dgc.apply_gradient(flat_out=memory, add_flat=True) and
                DGCCodec.compress(momentum_buffers=..., grads_in_memory=True)
  host_us       host wall time per step: `steps` steps queued, one synchronise, divided
  gpu_us        the same window between two device events
  launches      device activities (kernels + copies) of one step, from torch.profiler
  kernel_us_*   dispatch-attached time per step of param_sqnorm_kernel (+ finish),
                param_sgd_kernel and param_mask_kernel in (b)
(medians over `reps` windows after a warm-up window).

--norm-ab: the norm pass alone on the three layouts, per step, with the library as built
(default-policy loads) and with the `sqnorm_nt` variant of tools/build_variants.py
(non-temporal loads), each in a child process of its own (CHOCO_CODEC_LIB), and the same for the
norm pass followed by the update, whose re-read of p and g may hit the Infinity Cache.
"""
import argparse
import collections
import json
import math
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chocosgd_amd import build, codec, dgc  # noqa: E402
from chocosgd_amd.tensor_buffer import TensorBuffer  # noqa: E402

DEV = "cuda"
HP = {"lr": 0.1, "weight_decay": 1e-4, "momentum": 0.9, "dampening": 0.0, "nesterov": False}
CLIP, N_NODES, RATIO = 2.0, 4, 0.99
VARIANT = os.path.join(build.LIBDIR, "variants", "lib_sqnorm_nt.so")


def torch_loop(groups, state, thr):
    """DGC._apply_gradient with clip_grad, as torch runs it: one launch per op and tensor."""
    for group in groups:
        wd, mom, damp = group["weight_decay"], group["momentum"], group["dampening"]
        for p in group["params"]:
            d_p = p.grad.data
            if wd != 0:
                d_p.add_(p.data, alpha=wd)
            grad_norm = d_p.norm(p=2)
            if grad_norm >= thr:
                d_p = thr / grad_norm * d_p
            if mom != 0:
                st = state[p]
                if "momentum_buffer" not in st:
                    buf = st["momentum_buffer"] = torch.zeros_like(d_p)
                    buf.add_(d_p)
                else:
                    buf = st["momentum_buffer"]
                    buf.mul_(mom).add_(d_p, alpha=1 - damp)
                d_p = d_p.add(buf, alpha=mom) if group["nesterov"] else buf
            p.grad.data = d_p


def mask_loop(params, state, indices, k_per_seg, lens):
    """buf.mul_(nmask) per tensor (dgc.py:178-182) from the flat selection."""
    o = ko = 0
    for p, m, k in zip(params, lens, k_per_seg):
        buf = state[p]["momentum_buffer"]
        nmask = torch.ones_like(buf).view(-1)
        nmask[indices[ko:ko + k].long() - o] = 0.0
        buf.mul_(nmask.view_as(buf))
        o, ko = o + m, ko + k


def layouts():
    with open(os.path.join(ROOT, "tests", "golden", "layouts.json")) as f:
        r50 = json.load(f)["resnet50_imagenet"]
    return [("resnet50_fp32", r50, torch.float32), ("resnet50_bf16", r50, torch.bfloat16),
            ("t3000x100_fp32", [100] * 3000, torch.float32)]


def events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6, a.elapsed_time(b) / iters * 1e3


def median_of(fn, iters, reps):
    events(fn, max(2, iters // 10))  # warm-up: code objects, the allocator's blocks, first-step buffers
    runs = [events(fn, iters) for _ in range(reps)]
    return statistics.median(r[0] for r in runs), statistics.median(r[1] for r in runs)


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        cnt = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception as e:  # noqa: BLE001
        print(f"launch count not measured: {e}", file=sys.stderr)
        return None
    return cnt or None


def kernel_times(fn, names, iters=20):
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


def model(lens, dtype, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(m, generator=g, device=DEV).to(dtype)) for m in lens]
    for p in params:
        p.grad = (0.01 * torch.randn(p.shape, generator=g, device=DEV)).to(dtype)
    groups = [dict(HP, params=[p], name=f"p{i}") for i, p in enumerate(params)]
    mem = TensorBuffer([torch.zeros(m, device=DEV) for m in lens])
    cdc = dgc.DGCCodec(None, "compress_top_k", "gpu", N_NODES, strict_reference=False)
    return params, groups, mem, cdc, collections.defaultdict(dict)


def measure(name, lens, dtype, steps, reps):
    thr = CLIP * (1.0 / math.sqrt(N_NODES))
    pa, ga, ma, ca, sa = model(lens, dtype)

    def loop_step():
        torch_loop(ga, sa, thr)
        _, indices, _ = ca.compress([p.grad.data for p in pa], ma, RATIO)
        mask_loop(pa, sa, indices, ca.selected_shapes, lens)

    pb, gb, mb, cb, sb = model(lens, dtype)

    def fused_step():
        dgc.apply_gradient(gb, sb, clip_grad=True, clip_grad_val=CLIP, n_nodes=N_NODES, flat_out=mb, add_flat=True)
        cb.compress([p.grad.data for p in pb], mb, RATIO,
                    momentum_buffers=[sb[p]["momentum_buffer"] for p in pb], grads_in_memory=True)

    loop_host, loop_gpu = median_of(loop_step, steps, reps)
    fused_host, fused_gpu = median_of(fused_step, steps, reps)
    row = {"layout": name, "tensors": len(lens), "elements": sum(lens), "param_dtype": str(dtype).split(".")[-1],
           "steps": steps, "reps": reps,
           "loop_host_us": round(loop_host, 1), "loop_gpu_us": round(loop_gpu, 1),
           "loop_launches": count_launches(loop_step),
           "fused_host_us": round(fused_host, 1), "fused_gpu_us": round(fused_gpu, 1),
           "fused_launches": count_launches(fused_step)}
    kt = kernel_times(fused_step, ["param_sqnorm_kernel", "param_sqnorm_finish_kernel", "param_sgd_kernel",
                                   "param_mask_kernel"])
    for nm, (us, cnt) in kt.items():
        short = nm.replace("param_", "").replace("_kernel", "")
        row[f"kernel_us_{short}"], row[f"kernel_launches_{short}"] = us, cnt
    return row


def norm_rows(steps, reps):
    """The norm pass alone, and followed by the update (run in a child process per library)."""
    rows = []
    for name, lens, dtype in layouts():
        params, groups, mem, _, state = model(lens, dtype)
        datas, grads = [p.data for p in params], [p.grad.data for p in params]
        plan = codec.ParamSgdPlan(datas)

        def norm_only():
            codec.params_sqnorm(datas, grads, HP["weight_decay"], plan=plan)

        def norm_update():
            dgc.apply_gradient(groups, state, clip_grad=True, clip_grad_val=CLIP, n_nodes=N_NODES, flat_out=mem,
                               add_flat=True)

        row = {"norm_ab": name, "lib": os.path.basename(os.environ.get("CHOCO_CODEC_LIB") or "product")}
        row["norm_gpu_us"] = round(median_of(norm_only, steps, reps)[1], 1)
        row["norm_update_gpu_us"] = round(median_of(norm_update, steps, reps)[1], 1)
        kt = kernel_times(norm_update, ["param_sqnorm_kernel", "param_sgd_kernel"])
        row["kernel_us_sqnorm"], row["kernel_us_sgd"] = kt["param_sqnorm_kernel"][0], kt["param_sgd_kernel"][0]
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--norm-ab", action="store_true")
    ap.add_argument("--no-steps", action="store_true", help="skip the (a) / (b) rows (with --norm-ab)")
    ap.add_argument("--norm-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    if args.norm_child:
        norm_rows(args.steps, args.reps)
        return
    rows = []
    for name, lens, dtype in ([] if args.no_steps else layouts()):
        rows.append(measure(name, lens, dtype, args.steps, args.reps))
        print(json.dumps(rows[-1]), flush=True)
    if args.norm_ab:
        if not os.path.exists(VARIANT):
            sys.exit(f"{VARIANT} not built (tools/build_variants.py sqnorm_nt): no A/B")
        for lib in (None, VARIANT):
            env = dict(os.environ)
            env.pop("CHOCO_CODEC_LIB", None)
            if lib:
                env["CHOCO_CODEC_LIB"] = lib
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--norm-child", "--steps", str(args.steps),
                                "--reps", str(args.reps)], env=env, capture_output=True, text=True, timeout=300)
            sys.stderr.write(r.stderr[-2000:])
            if r.returncode:
                # a child that failed on the device: nothing more is started on it, nothing is written
                sys.exit(f"the norm A/B child for {os.path.basename(lib or 'the product library')} ended with "
                         f"status {r.returncode}; stopping")
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    rows.append(json.loads(line))
                    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
