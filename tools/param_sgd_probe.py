"""Cost of the optimizer update in front of a CHOCO step, and its parity with torch's own ops.

    python tools/param_sgd_probe.py [--out FILE] [--steps 100] [--reps 5]

Timing rows (one JSON line per layout: ResNet-50 in fp32 and in bf16, 3000 tensors of 100
elements; each parameter its own allocation; weight decay + momentum, no Nesterov):
  (a) loop_*    what runs without the batched kernel: apply_gradient as one torch op per line
                and tensor (written out below with torch alone, so that any commit of this
                repository can run it), then utils.recover_params(get_hat_params=False)
  (b) fused_*   utils.apply_gradient(..., flat_out=flat): the update and the pack in one launch
                per chunk of tensors
  (c) master_*  utils.apply_gradient(..., master=mw): the update on the persistent fp32 master
                copy with fp32 momentum buffers, the params written narrowed, one launch per
                chunk of tensors (param_sgd_master_kernel); its yardstick is the fp32 layout's
                kernel_tbps_sgd of the same run
  host_us       host wall time per step: `steps` steps queued, one synchronise, divided
  gpu_us        the same window between two device events
  launches      device activities (kernels + copies) of one step, from torch.profiler
  kernel_us_*, kernel_tbps_*   dispatch-attached time of param_sgd_kernel (in (b)) and of
                param_pack_kernel (in (a)), and the bytes each moves divided by it
(medians over `reps` windows after a warm-up window).

All-reduce rows (--rows allreduce, or with everything else by default; one JSON line per layout:
ResNet-50 in fp32, in bf16 and in bf16 with master weights, 3000 tensors of 100 elements), the
centralized SGD step with a loopback aggregator (_agg returns the buffer, world size 1.0):
  step_*     utils.allreduce_sgd_step: one pack launch and one update launch per chunk
             (param_sgd_flatgrad_kernel / param_sgd_master_flatgrad_kernel)
  parent_*   the four passes it replaces: codec.params_pack of the gradients, a torch divide that
             allocates a new flat buffer, TensorBuffer.unpack into p.grad, utils.apply_gradient
             (master: apply_gradient(master=mw), which sees the rounded gradients)
  kernel_us_update / kernel_tbps_update: the new update kernel alone, against bytes_update;
  kernel_us_step: pack + update; kernel_us_parent: pack + unpack + the SGD kernel, dispatch
  attached, plus div_gpu_us, the torch divide alone between two device events.

Clip / loss-scale rows of the all-reduce step (--rows allreduce_scaled only; ResNet-50 in fp32
with clip_norm, in fp16 with loss_scale + clip_norm, and that with master weights; the same
loopback aggregator), both columns in the same process:
  step_*     utils.allreduce_sgd_step(clip_norm=, loss_scale=): the norm pass, the scaled pack
             with the flag slot, one small launch for the scale, the update
  parent_*   what runs without it: torch._amp_foreach_non_finite_check_and_unscale_, a loopback
             "all-reduce" of found_inf and its .item(), utils.clip_grad_norm_, today's
             allreduce_sgd_step, torch._amp_update_scale_ (the fp32 row: the clip and the step)
  kernel_us_step / kernel_us_parent: this library's kernels of one step, dispatch attached and
             summed, plus torch_gpu_us, torch's two _amp_* ops alone between two device events;
  kernel_ratio, host_ratio: step / parent; beats_parent_*: whether the ratio is under 0.9, the
             box-to-box spread of about 10 %.
The loss scale is 1.0 with growth switched off and the gradients are rewritten by every step
(the averaged gradient), so the values settle; the time does not depend on them.

Stochastic-rounding row (--sr [--runs 5], alone): ResNet-50 in bf16, the kernel time of the plain
update, of the master update and of the stochastic-rounding update, `runs` measurements each and
their range, every column on a model of its own, alone on the device (measure_sr); run from a tree without stochastic rounding it
reports the first two, the other column of an A/B visit.

Parity rows: elements of p, buf and flat on which three steps of the kernel differ from the
same three steps of torch's own op sequence on the device, per dtype, on the fixture layout
(tests/golden/sgd_inputs.npz) and on one tensor of 2^20 elements.
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chocosgd_amd import codec, utils  # noqa: E402

DEV = "cuda"
HP = {"lr": 0.1, "weight_decay": 1e-4, "momentum": 0.9, "dampening": 0.0, "nesterov": False}


def torch_loop(groups, state):
    """apply_gradient (apply mode) as torch runs it: in-place ops, one launch each."""
    for group in groups:
        wd, mom, damp = group["weight_decay"], group["momentum"], group["dampening"]
        for p in group["params"]:
            d_p = p.grad.data
            if wd != 0:
                d_p.add_(p.data, alpha=wd)
            if mom != 0:
                st = state[p]
                if "momentum_buffer" not in st:
                    buf = st["momentum_buffer"] = torch.zeros_like(p.data)
                    buf.mul_(mom).add_(d_p)
                else:
                    buf = st["momentum_buffer"]
                    buf.mul_(mom).add_(d_p, alpha=1 - damp)
                d_p = d_p.add(buf, alpha=mom) if group["nesterov"] else buf
            p.data.add_(d_p, alpha=-group["lr"])


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


def kernel_time(fn, name, iters=20):
    """Dispatch-attached time of kernel `name` per call of fn (us, all its launches summed)."""
    codec.profile_reset()
    codec.profile_filter([name])
    codec.profile_enable(True)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    codec.profile_enable(False)
    t, c = codec.profile_read(name)
    codec.profile_filter(None)
    codec.profile_reset()
    return (t / iters * 1e3, c // iters) if c else (None, 0)


def model(lens, dtype, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(m, generator=g, device=DEV).to(dtype)) for m in lens]
    for p in params:
        p.grad = (0.01 * torch.randn(p.shape, generator=g, device=DEV)).to(dtype)
    groups = [dict(HP, params=[p], name=f"p{i}") for i, p in enumerate(params)]
    return params, groups, list(enumerate(gr["name"] for gr in groups))


def measure(name, lens, dtype, steps, reps):
    n, esz = sum(lens), torch.empty(0, dtype=dtype).element_size()
    pa, ga, na = model(lens, dtype)
    sa = collections.defaultdict(dict)

    def loop_step():
        torch_loop(ga, sa)
        utils.recover_params(ga, na, get_hat_params=False)

    pb, gb, _ = model(lens, dtype)
    sb = collections.defaultdict(dict)
    flat = torch.empty(n, device=DEV)

    def fused_step():
        utils.apply_gradient(gb, sb, flat_out=flat)

    pm, gm, nm = model(lens, dtype)
    sm = collections.defaultdict(dict)
    mw = utils.MasterWeights(gm, nm)

    def master_step():
        utils.apply_gradient(gm, sm, master=mw)

    loop_host, loop_gpu = median_of(loop_step, steps, reps)
    fused_host, fused_gpu = median_of(fused_step, steps, reps)
    master_host, master_gpu = median_of(master_step, steps, reps)
    sgd_bytes = n * (5 * esz + 4)   # reads p, g, buf; writes buf, p and the fp32 flat
    master_bytes = n * (2 * esz + 16)  # reads master, g, the fp32 buf; writes buf, master and p
    pack_bytes = n * (esz + 4)
    k_sgd, l_sgd = kernel_time(fused_step, "param_sgd_kernel")
    k_pack, l_pack = kernel_time(loop_step, "param_pack_kernel")
    k_master, l_master = kernel_time(master_step, "param_sgd_master_kernel")
    row = {"layout": name, "tensors": len(lens), "elements": n, "param_dtype": str(dtype).split(".")[-1],
           "steps": steps, "reps": reps,
           "loop_host_us": round(loop_host, 1), "loop_gpu_us": round(loop_gpu, 1), "loop_launches": count_launches(loop_step),
           "fused_host_us": round(fused_host, 1), "fused_gpu_us": round(fused_gpu, 1),
           "fused_launches": count_launches(fused_step), "sgd_bytes": sgd_bytes, "pack_bytes": pack_bytes,
           "master_host_us": round(master_host, 1), "master_gpu_us": round(master_gpu, 1),
           "master_launches": count_launches(master_step), "master_bytes": master_bytes}
    if k_master:
        row.update(kernel_us_master=round(k_master, 2), kernel_launches_master=l_master,
                   kernel_tbps_master=round(master_bytes / k_master / 1e6, 3))
    if k_sgd:
        row.update(kernel_us_sgd=round(k_sgd, 2), kernel_launches_sgd=l_sgd,
                   kernel_tbps_sgd=round(sgd_bytes / k_sgd / 1e6, 3))
    if k_pack:
        row.update(kernel_us_pack=round(k_pack, 2), kernel_launches_pack=l_pack,
                   kernel_tbps_pack=round(pack_bytes / k_pack / 1e6, 3))
    return row


class _Loopback:
    """The aggregator of a single process: the sum is the buffer itself; the world size only
    sets the divisor (1.0: the gradients keep their magnitude over the timed steps; the kernel
    divides all the same)."""
    world_size = 1.0

    def _agg(self, data, op=None, distributed=True):
        return data


def measure_allreduce(name, lens, dtype, master, steps, reps):
    from chocosgd_amd.tensor_buffer import TensorBuffer
    n, esz = sum(lens), torch.empty(0, dtype=dtype).element_size()
    agg = _Loopback()
    pa, ga, na = model(lens, dtype)
    sa = collections.defaultdict(dict)
    mwa = utils.MasterWeights(ga, na) if master else None

    def new_step():
        utils.allreduce_sgd_step(ga, na, sa, agg, master=mwa)

    pb, gb, nb = model(lens, dtype)
    sb = collections.defaultdict(dict)
    mwb = utils.MasterWeights(gb, nb) if master else None
    grads = [p.grad for p in pb]
    sizes = [g.size() for g in grads]
    flat = torch.empty(n, device=DEV)

    def parent_step():
        codec.params_pack(grads, flat)
        avg = agg._agg(flat, op="sum") / agg.world_size
        TensorBuffer.from_flat(avg, sizes).unpack(grads)
        utils.apply_gradient(gb, sb, master=mwb)

    step_host, step_gpu = median_of(new_step, steps, reps)
    parent_host, parent_gpu = median_of(parent_step, steps, reps)
    _, div_gpu = median_of(lambda: flat / agg.world_size, steps, reps)
    upd = "param_sgd_master_flatgrad_kernel" if master else "param_sgd_flatgrad_kernel"
    old = "param_sgd_master_kernel" if master else "param_sgd_kernel"
    bytes_update = n * ((20 + 2 * esz) if master else (4 + 5 * esz))  # with the grad write
    bytes_parent = n * (esz + 4) + n * 8 + n * (4 + esz) + (n * (2 * esz + 16) if master else n * 5 * esz)
    k_upd, l_upd = kernel_time(new_step, upd)
    k_pack, l_pack = kernel_time(new_step, "param_pack_kernel")
    k_ppack, _ = kernel_time(parent_step, "param_pack_kernel")
    k_unpack, _ = kernel_time(parent_step, "param_unpack_kernel")
    k_old, l_old = kernel_time(parent_step, old)
    row = {"allreduce": name, "tensors": len(lens), "elements": n, "param_dtype": str(dtype).split(".")[-1],
           "master": master, "steps": steps, "reps": reps,
           "step_host_us": round(step_host, 1), "step_gpu_us": round(step_gpu, 1),
           "step_launches": count_launches(new_step), "bytes_update": bytes_update,
           "bytes_step": bytes_update + n * (esz + 4),
           "parent_host_us": round(parent_host, 1), "parent_gpu_us": round(parent_gpu, 1),
           "parent_launches": count_launches(parent_step), "bytes_parent": bytes_parent,
           "div_gpu_us": round(div_gpu, 2)}
    if k_upd and k_pack:
        row.update(kernel_us_update=round(k_upd, 2), kernel_launches_update=l_upd,
                   kernel_tbps_update=round(bytes_update / k_upd / 1e6, 3), kernel_us_pack=round(k_pack, 2),
                   kernel_us_step=round(k_upd + k_pack, 2))
    if k_ppack and k_unpack and k_old:
        row.update(kernel_us_parent_pack=round(k_ppack, 2), kernel_us_parent_unpack=round(k_unpack, 2),
                   kernel_us_parent_sgd=round(k_old, 2), kernel_launches_parent_sgd=l_old,
                   kernel_us_parent=round(k_ppack + k_unpack + k_old + div_gpu, 2))
    return row


def measure_allreduce_scaled(name, lens, dtype, master, scaled, steps, reps, max_norm=0.4):
    n = sum(lens)
    agg = _Loopback()
    pa, ga, na = model(lens, dtype)
    sa = collections.defaultdict(dict)
    mwa = utils.MasterWeights(ga, na) if master else None
    scaler = utils.LossScaler(DEV, init_scale=1.0, growth_interval=1 << 30) if scaled else None

    def new_step():
        utils.allreduce_sgd_step(ga, na, sa, agg, master=mwa, clip_norm=max_norm, loss_scale=scaler)

    pb, gb, nb = model(lens, dtype)
    sb = collections.defaultdict(dict)
    mwb = utils.MasterWeights(gb, nb) if master else None
    grads = [p.grad for p in pb]
    scale_b, tracker_b = torch.ones(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    found = torch.zeros(1, device=DEV)

    def torch_ops():
        found.zero_()
        torch._amp_foreach_non_finite_check_and_unscale_(grads, found, scale_b.double().reciprocal().float())
        torch._amp_update_scale_(scale_b, tracker_b, found, 2.0, 0.5, 1 << 30)

    def parent_step():
        skip = False
        if scaled:
            found.zero_()
            torch._amp_foreach_non_finite_check_and_unscale_(grads, found, scale_b.double().reciprocal().float())
            skip = bool(agg._agg(found, op="sum").item())  # the second collective and its host sync
        if not skip:
            utils.clip_grad_norm_(pb, max_norm)
            utils.allreduce_sgd_step(gb, nb, sb, agg, master=mwb)
        if scaled:
            torch._amp_update_scale_(scale_b, tracker_b, found, 2.0, 0.5, 1 << 30)

    step_host, step_gpu = median_of(new_step, steps, reps)
    parent_host, parent_gpu = median_of(parent_step, steps, reps)
    torch_gpu = median_of(torch_ops, steps, reps)[1] if scaled else 0.0
    tail = "_scaled_kernel" if scaled else "_kernel"
    upd = "param_sgd_master_flatgrad" if master else "param_sgd_flatgrad"
    new_names = ["param_sqnorm_kernel", "param_gradnorm_scaled_local_total_kernel" if scaled
                 else "param_gradnorm_total_kernel", "param_pack_scaled_kernel", upd + tail]
    new_names += ["loss_scale_update_kernel"] if scaled else []
    old_names = ["param_sqnorm_kernel", "param_gradnorm_total_kernel", "param_sgd_gclip_kernel", "param_pack_kernel",
                 upd + "_kernel"]
    k_new = {nm: kernel_time(new_step, nm)[0] for nm in new_names}
    k_old = {nm: kernel_time(parent_step, nm)[0] for nm in old_names}
    row = {"allreduce_scaled": name, "tensors": len(lens), "elements": n, "param_dtype": str(dtype).split(".")[-1],
           "master": master, "loss_scale": scaled, "clip_norm": max_norm, "steps": steps, "reps": reps,
           "step_host_us": round(step_host, 1), "step_gpu_us": round(step_gpu, 1),
           "step_launches": count_launches(new_step),
           "parent_host_us": round(parent_host, 1), "parent_gpu_us": round(parent_gpu, 1),
           "parent_launches": count_launches(parent_step), "torch_gpu_us": round(torch_gpu, 2),
           "host_ratio": round(step_host / parent_host, 3), "beats_parent_host": step_host < 0.9 * parent_host,
           "kernels_step": {nm: None if t is None else round(t, 2) for nm, t in k_new.items()},
           "kernels_parent": {nm: None if t is None else round(t, 2) for nm, t in k_old.items()}}
    if all(k_new.values()) and all(k_old.values()):
        ks, kp = sum(k_new.values()), sum(k_old.values()) + torch_gpu
        row.update(kernel_us_step=round(ks, 2), kernel_us_parent=round(kp, 2), kernel_ratio=round(ks / kp, 3),
                   beats_parent_kernels=ks < 0.9 * kp)
    return row


def allreduce_scaled_layouts():
    with open(os.path.join(ROOT, "tests", "golden", "layouts.json")) as f:
        r50 = json.load(f)["resnet50_imagenet"]
    return [("resnet50_fp32_clip", r50, torch.float32, False, False),
            ("resnet50_fp16_scaled", r50, torch.float16, False, True),
            ("resnet50_fp16_scaled_master", r50, torch.float16, True, True)]


def allreduce_layouts():
    with open(os.path.join(ROOT, "tests", "golden", "layouts.json")) as f:
        r50 = json.load(f)["resnet50_imagenet"]
    return [("resnet50_fp32", r50, torch.float32, False), ("resnet50_bf16", r50, torch.bfloat16, False),
            ("resnet50_bf16_master", r50, torch.bfloat16, True), ("t3000x100_fp32", [100] * 3000, torch.float32, False)]


def measure_sr(lens, runs, iters=20):
    """--sr: the three ways to update a bf16 ResNet-50, dispatch-attached kernel time per step,
    `runs` measurements of `iters` steps each and their range: the plain update
    (param_sgd_kernel, with the flat output), the master update (param_sgd_master_kernel) and,
    where the library has it, the stochastic-rounding update (param_sgd_sr_kernel, with the flat
    output: the plain update's traffic).  A tree without stochastic rounding reports the first
    two: the parent's column of an A/B visit."""
    n = sum(lens)
    dtype = torch.bfloat16

    def case(name):
        """The step of one column and its kernel, on a model of its own."""
        params, groups, names = model(lens, dtype)
        state = collections.defaultdict(dict)
        if name == "master":
            mw = utils.MasterWeights(groups, names)
            return (lambda: utils.apply_gradient(groups, state, master=mw)), "param_sgd_master_kernel"
        flat = torch.empty(n, device=DEV)
        if name == "plain":
            return (lambda: utils.apply_gradient(groups, state, flat_out=flat)), "param_sgd_kernel"
        sr = utils.StochasticRounding(5)
        return (lambda: utils.apply_gradient(groups, state, flat_out=flat, rounding=sr)), "param_sgd_sr_kernel"

    columns = ["plain", "master"] + (["sr"] if hasattr(utils, "StochasticRounding") else [])
    row = {"sr_update": "resnet50_bf16", "tensors": len(lens), "elements": n, "runs": runs, "iters": iters,
           "bytes_plain": n * 14, "bytes_master": n * 20, "bytes_sr": n * 14}
    times = {}
    # one column at a time, the only model on the device while it is measured: the allocator hands every
    # tree, and every column, the same addresses (with a third model alive the master update of the same code
    # measured 3.5 % slower)
    for name in columns:
        fn, kernel = case(name)
        for _ in range(3):  # warm-up: code objects, first-step buffers
            fn()
        times[name] = []
        for _ in range(runs):
            t, launches = kernel_time(fn, kernel, iters)
            times[name].append(round(t, 2))
            row[f"kernel_launches_{name}"] = launches
        del fn
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    for name, ts in times.items():
        row[f"kernel_us_{name}"] = ts
        row[f"kernel_us_{name}_range"] = [min(ts), max(ts)]
        row[f"kernel_tbps_{name}"] = round(row[f"bytes_{name}"] / statistics.median(ts) / 1e6, 3)
    return row


def _differ(a, b):
    a, b = a.float().reshape(-1), b.float().reshape(-1)
    same = (a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))
    return int((~same).sum().item())


def parity(name, p0, gs, lens, dtype):
    """Three steps of the kernel against three steps of torch's ops, from the same inputs."""
    def build():
        params, o = [], 0
        for m in lens:
            params.append(torch.nn.Parameter(p0[o:o + m].clone().to(dtype)))
            o += m
        return params, [dict(HP, params=[p]) for p in params]

    def set_grads(params, g):
        o = 0
        for p, m in zip(params, lens):
            p.grad = g[o:o + m].clone().to(dtype)
            o += m

    (pk, gk), (pt, gt) = build(), build()
    sk, st = collections.defaultdict(dict), collections.defaultdict(dict)
    flat = torch.empty(sum(lens), device=DEV)
    row = {"parity": name, "dtype": str(dtype).split(".")[-1], "elements": sum(lens)}
    for k, g in enumerate(gs):
        set_grads(pk, g)
        set_grads(pt, g)
        utils.apply_gradient(gk, sk, flat_out=flat)
        torch_loop(gt, st)
        cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])  # noqa: E731
        row[f"step{k}"] = {"p": _differ(cat(pk), cat(pt)),
                           "buf": _differ(cat([sk[p]["momentum_buffer"] for p in pk]),
                                          cat([st[p]["momentum_buffer"] for p in pt])),
                           "flat": _differ(flat, cat(pt).float())}
    return row


def parity_rows():
    with np.load(os.path.join(ROOT, "tests", "golden", "sgd_inputs.npz")) as z:
        lens = z["lens"].tolist()
        p0 = torch.from_numpy(z["p0"]).to(DEV)
        gs = [torch.from_numpy(z[f"g{k}"]).to(DEV) for k in range(3)]
    g = torch.Generator(device=DEV).manual_seed(11)
    m = 1 << 20
    big_p = torch.randn(m, generator=g, device=DEV)
    big_g = [0.01 * torch.randn(m, generator=g, device=DEV) for _ in range(3)]
    rows = []
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        rows.append(parity("fixture_layout", p0, gs, lens, dtype))
        rows.append(parity("one_tensor_1M", big_p, big_g, [m], dtype))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", choices=["all", "allreduce", "allreduce_scaled"], default="all")
    ap.add_argument("--sr", action="store_true", help="only the stochastic-rounding row (see measure_sr)")
    ap.add_argument("--runs", type=int, default=5, help="--sr: measurements per column")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a ROCm device"
    rows = []
    kind = "sr" if args.sr else args.rows
    if kind == "sr":
        rows.append(measure_sr(layouts()[1][1], args.runs))
        print(json.dumps(rows[-1]), flush=True)
    for name, lens, dtype, master, scaled in (allreduce_scaled_layouts() if kind == "allreduce_scaled" else []):
        rows.append(measure_allreduce_scaled(name, lens, dtype, master, scaled, args.steps, args.reps))
        print(json.dumps(rows[-1]), flush=True)
    for name, lens, dtype in (layouts() if kind in ("all", "allreduce") else []):
        # the fp32 ResNet-50 row stays in an all-reduce run: its kernel_tbps_sgd is the yardstick
        if kind == "all" or name == "resnet50_fp32":
            rows.append(measure(name, lens, dtype, args.steps, args.reps))
            print(json.dumps(rows[-1]), flush=True)
    for name, lens, dtype, master in (allreduce_layouts() if kind in ("all", "allreduce") else []):
        rows.append(measure_allreduce(name, lens, dtype, master, args.steps, args.reps))
        print(json.dumps(rows[-1]), flush=True)
    for row in (parity_rows() if kind == "all" else []):
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
