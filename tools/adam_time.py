"""Time of one Adam / AdamW update of a whole model: the batched kernels (csrc/adam.hip) against
torch's own optimizers on the same tensors, in the same process.

    python tools/adam_time.py [--out FILE] [--updates 20] [--warmup 5] [--reps 5] [--sr]

One JSON line per layout (ResNet-50's 161 tensors in bf16 and in fp32; each parameter its own
allocation).  A window is `updates` updates between two device events after `warmup` updates;
the ways alternate window by window, and the medians over `reps` windows are reported, with the
spread (min, max) beside them:
  plain         param_adam_kernel with the flat output and no parameter write: the CHOCO form
                (ParamAdamPlan.run(flat, write=False))
  plain_write   the same with the parameters written and no flat output: torch's own job
  master        param_adam_master_kernel on the flat fp32 copy with fp32 moments, parameters
                written (over a bf16 model; over an fp32 one it has no use and is skipped)
  fused         torch.optim.AdamW(fused=True).step() -- the yardstick: what a user has today
  fused_pack    ... followed by codec.params_pack of the new parameters (param_pack_kernel):
                what the CHOCO form replaces
  foreach       torch.optim.AdamW(foreach=True).step()
*_us is device time per update, *_bytes the algorithmic bytes of one update (every operand read
once and written once), *_tbps their quotient, *_hbm that over the 8.0 TB/s of the data sheet.
kernel_us_*: the dispatch-attached time of the kernel's launches alone (the library's profile
hooks), in a window of its own.  Needs a ROCm device; there is no fall-back.

--sr: the three ways to run Adam on a bf16 model instead, ResNet-50 in bf16 only, same windows:
  plain_write   param_adam_kernel, parameters written, no flat output (14 B per element)
  sr_write      param_adam_sr_kernel (ParamAdamPlan.run(sr=)), parameters written, no flat (14 B)
  master        param_adam_master_kernel, parameters written (28 B)
  plain, sr     the CHOCO form of the first two: flat written, parameters not (16 B)
with the ratios sr_write_vs_plain_write, sr_vs_plain and sr_write_vs_master (the last one must
be below 1: the stochastic kernel moves half the master kernel's bytes).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import param_sgd_probe as P  # noqa: E402
from chocosgd_amd import codec  # noqa: E402

DEV = P.DEV
HBM_TBPS = 8.0
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


def layouts():
    with open(os.path.join(ROOT, "tests", "golden", "layouts.json")) as f:
        r50 = json.load(f)["resnet50_imagenet"]
    return [("resnet50_bf16", r50, torch.bfloat16), ("resnet50_fp32", r50, torch.float32)]


def tensors(lens, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(m, generator=g, device=DEV).to(dtype)) for m in lens]
    for p in params:
        p.grad = (0.01 * torch.randn(p.shape, generator=g, device=DEV)).to(dtype)
    return params


class Ours:
    """One plan over its own tensors, the tables written once; step() advances the counts."""

    def __init__(self, lens, dtype, master):
        self.params = tensors(lens, dtype, 0)
        mdt = torch.float32 if master else dtype
        self.m = [torch.zeros_like(p.data, dtype=mdt) for p in self.params]
        self.v = [torch.zeros_like(p.data, dtype=mdt) for p in self.params]
        self.plan = plan = codec.ParamAdamPlan(self.params)
        self.n = plan.n
        self.flat = torch.cat([p.detach().float().reshape(-1) for p in self.params])
        self.count = 0
        for i, p in enumerate(self.params):
            plan.param_ptrs[i], plan.grad_ptrs[i] = p.data_ptr(), p.grad.data_ptr()
            plan.exp_avg_ptrs[i], plan.exp_avg_sq_ptrs[i] = self.m[i].data_ptr(), self.v[i].data_ptr()
            plan.flags[i] = codec.ADAM_F_DECOUPLED
            plan.lr[i], (plan.beta1[i], plan.beta2[i]) = HP["lr"], HP["betas"]
            plan.eps[i], plan.weight_decay[i] = HP["eps"], HP["weight_decay"]

    def _advance(self):
        self.count += 1
        for i in range(self.plan.nseg):
            self.plan.step[i] = self.count

    def plain(self):
        self._advance()
        self.plan.run(self.flat, write=False)

    def plain_write(self):
        self._advance()
        self.plan.run(None, write=True)

    def master(self):
        self._advance()
        self.plan.run_master(self.flat, write=True)

    def sr(self):
        self._advance()
        self.plan.run(self.flat, write=False, sr=(7, self.count))

    def sr_write(self):
        self._advance()
        self.plan.run(None, write=True, sr=(7, self.count))


def measure(name, lens, dtype, updates, warmup, reps):
    n, esz = sum(lens), torch.empty(0, dtype=dtype).element_size()
    a, b = Ours(lens, dtype, False), Ours(lens, dtype, False)
    ways = {"plain": a.plain, "plain_write": b.plain_write}
    nbytes = {"plain": n * (6 * esz + 4), "plain_write": n * 7 * esz, "fused": n * 7 * esz, "foreach": None,
              "fused_pack": n * (7 * esz + esz + 4), "master": n * (8 + 2 * esz + 16)}
    if dtype != torch.float32:
        ways["master"] = Ours(lens, dtype, True).master
    pf, pe = tensors(lens, dtype, 0), tensors(lens, dtype, 0)
    fused = torch.optim.AdamW(pf, fused=True, **HP)
    foreach = torch.optim.AdamW(pe, foreach=True, **HP)
    flat = torch.empty(n, device=DEV)

    def fused_pack():
        fused.step()
        codec.params_pack([p.data for p in pf], flat)

    ways.update({"fused": fused.step, "fused_pack": fused_pack, "foreach": foreach.step})
    row = {"layout": name, "tensors": len(lens), "elements": n, "param_dtype": str(dtype).split(".")[-1],
           "updates": updates, "warmup": warmup, "reps": reps}
    for fn in ways.values():
        P.events(fn, warmup)
    runs = {tag: [] for tag in ways}
    for _ in range(reps):
        for tag, fn in ways.items():
            runs[tag].append(P.events(fn, updates)[1])
    for tag in ways:
        t = statistics.median(runs[tag])
        row[f"{tag}_us"] = round(t, 1)
        row[f"{tag}_us_min_max"] = [round(min(runs[tag]), 1), round(max(runs[tag]), 1)]
        if nbytes[tag]:
            row[f"{tag}_bytes"] = nbytes[tag]
            row[f"{tag}_tbps"] = round(nbytes[tag] / t / 1e6, 3)
            row[f"{tag}_hbm"] = round(nbytes[tag] / t / 1e6 / HBM_TBPS, 3)
        row[f"{tag}_launches"] = P.count_launches(ways[tag])
    for tag, kernel in (("plain", "param_adam_kernel"), ("master", "param_adam_master_kernel")):
        if tag in ways:
            t, launches = P.kernel_time(ways[tag], kernel, updates)
            if t:
                row.update({f"kernel_us_{tag}": round(t, 2), f"kernel_launches_{tag}": launches,
                            f"kernel_tbps_{tag}": round(nbytes[tag] / t / 1e6, 3)})
    row["plain_vs_fused"] = round(row["fused_us"] / row["plain_us"], 3)
    row["plain_vs_fused_pack"] = round(row["fused_pack_us"] / row["plain_us"], 3)
    return row


def measure_sr(name, lens, updates, warmup, reps):
    """The three ways on the bf16 layout, every way on a model of its own."""
    dtype = torch.bfloat16
    n = sum(lens)
    ways = {"plain_write": Ours(lens, dtype, False).plain_write, "sr_write": Ours(lens, dtype, False).sr_write,
            "master": Ours(lens, dtype, True).master, "plain": Ours(lens, dtype, False).plain,
            "sr": Ours(lens, dtype, False).sr}
    nbytes = {"plain_write": n * 14, "sr_write": n * 14, "master": n * 28, "plain": n * 16, "sr": n * 16}
    kernels = {"plain_write": "param_adam_kernel", "sr_write": "param_adam_sr_kernel",
               "master": "param_adam_master_kernel", "plain": "param_adam_kernel", "sr": "param_adam_sr_kernel"}
    row = {"layout": name, "tensors": len(lens), "elements": n, "param_dtype": "bfloat16", "updates": updates,
           "warmup": warmup, "reps": reps}
    for fn in ways.values():
        P.events(fn, warmup)
    runs = {tag: [] for tag in ways}
    for _ in range(reps):
        for tag, fn in ways.items():
            runs[tag].append(P.events(fn, updates)[1])
    for tag in ways:
        t = statistics.median(runs[tag])
        row[f"{tag}_us"] = round(t, 1)
        row[f"{tag}_us_min_max"] = [round(min(runs[tag]), 1), round(max(runs[tag]), 1)]
        row[f"{tag}_bytes"] = nbytes[tag]
        row[f"{tag}_tbps"] = round(nbytes[tag] / t / 1e6, 3)
    for tag, fn in ways.items():
        t, launches = P.kernel_time(fn, kernels[tag], updates)
        if t:
            row.update({f"kernel_us_{tag}": round(t, 2), f"kernel_launches_{tag}": launches})
    row["sr_write_vs_plain_write"] = round(row["sr_write_us"] / row["plain_write_us"], 3)
    row["sr_vs_plain"] = round(row["sr_us"] / row["plain_us"], 3)
    row["sr_write_vs_master"] = round(row["sr_write_us"] / row["master_us"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sr", action="store_true", help="plain, stochastic and master Adam on the bf16 layout")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the timer needs a ROCm device"
    rows = []
    for name, lens, dtype in layouts():
        if args.sr and dtype != torch.bfloat16:
            continue
        if args.sr:
            rows.append(measure_sr(name, lens, args.updates, args.warmup, args.reps))
        else:
            rows.append(measure(name, lens, dtype, args.updates, args.warmup, args.reps))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
