"""Time of the majority-vote signSGD kernels (csrc/vote.hip, csrc/signstep.hip) against the
sequence they replace, in the same process, alternated.

    python tools/sign_vote_time.py [--out FILE] [--iters 20] [--warmup 5] [--reps 5] [--voters 8]

One JSON line per layout (ResNet-50's 161 tensors, 25,557,032 elements, in fp32 and in bf16; each
parameter its own allocation), W = 8 voters:
  new        codec.sign_vote + ParamSgdPlan.sign_step: 9 N' 4 + (2 esz n + N' 4) bytes
  old        the decode-sum-repack majority vote (W sign_unpack, W - 1 torch adds, one sign pack),
             sign_unpack of the verdict into a flat buffer, params_ef(APPLY | SCALE)
  ef         params_ef(APPLY | SCALE) alone: the flat-tile kernel on the same layout (4 more bytes
             per element than the packed-sign step)
  fused      sign_sgd.fused_step whole -- grad-mode SGD, pack, vote, step -- with a loopback
             gather that hands back prepared messages (the gather excluded); for the record
*_us is device time per call between two events (`iters` calls a window after `warmup`, the ways
alternating window by window; the median over `reps` windows, min and max beside it).
kernel_us_*: the dispatch-attached time of the kernel's launches alone (the library's profile
hooks), summed over a call's launches, in a window of its own; *_tbps against the algorithmic
bytes.  new_vs_old = old_us / new_us must be at least 4.  CHOCO_CODEC_LIB picks another build of
the library (tools/build_variants.py signstep_aligned); the row's "lib" names it.
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
from chocosgd_amd import _lib, codec, sign_sgd  # noqa: E402

DEV = P.DEV
LR = 0.01


class Prepared:
    """A loopback all_gather: this rank's message and W - 1 prepared ones."""

    def __init__(self, others):
        self.others = others

    def _agg(self, data, communication_scheme=None, async_op=False):
        return [data] + self.others


def measure(name, lens, dtype, W, iters, warmup, reps):
    n, esz = sum(lens), torch.empty(0, dtype=dtype).element_size()
    Np = codec.sign_words(n)
    g = torch.Generator(device=DEV).manual_seed(0)
    msgs = [codec.sign_compress(torch.randn(n, generator=g, device=DEV), want_norms=False)[0] for _ in range(W)]
    verdict = torch.empty(Np, dtype=torch.int32, device=DEV)
    models = {}
    for tag in ("new", "old", "ef", "fused"):
        params, groups, names = P.model(lens, dtype)
        plan = codec.ParamSgdPlan(params)
        for i, p in enumerate(params):
            plan.param_ptrs[i], plan.lr[i] = p.data_ptr(), LR
        models[tag] = (params, groups, names, plan)
    flat = torch.randn(n, generator=g, device=DEV)

    def new():
        models["new"][3].sign_step(codec.sign_vote(msgs, out=verdict))

    def old():
        total = None
        for t in msgs:
            dec = codec.sign_unpack(t, 32 * Np)
            total = dec if total is None else total + dec
        packed, _ = codec.sign_compress(total, want_norms=False)
        models["old"][3].ef(codec.sign_unpack(packed, n), codec.EF_APPLY | codec.EF_SCALE, lr=LR)

    def ef():
        models["ef"][3].ef(flat, codec.EF_APPLY | codec.EF_SCALE, lr=LR)

    _, fgroups, fnames, _ = models["fused"]
    fstate = collections.defaultdict(dict)
    comp = sign_sgd.MajorityVoteCompressor(0, W, Prepared(msgs[1:]), "gpu")

    def fused():
        sign_sgd.fused_step(comp, fgroups, fnames, fstate)

    ways = {"new": new, "old": old, "ef": ef, "fused": fused}
    nbytes = {"new": 9 * Np * 4 + 2 * esz * n + Np * 4, "ef": (2 * esz + 4) * n}
    row = {"layout": name, "tensors": len(lens), "elements": n, "param_dtype": str(dtype).split(".")[-1], "voters": W,
           "iters": iters, "warmup": warmup, "reps": reps, "lib": os.path.basename(_lib.LIB_PATH)}
    for fn in ways.values():
        P.events(fn, warmup)
    runs = {tag: [] for tag in ways}
    for _ in range(reps):
        for tag, fn in ways.items():
            runs[tag].append(P.events(fn, iters)[1])
    for tag in ways:
        t = statistics.median(runs[tag])
        row[f"{tag}_us"] = round(t, 1)
        row[f"{tag}_us_min_max"] = [round(min(runs[tag]), 1), round(max(runs[tag]), 1)]
        if tag in nbytes:
            row[f"{tag}_bytes"] = nbytes[tag]
            row[f"{tag}_tbps"] = round(nbytes[tag] / t / 1e6, 3)
    kernels = {"sign_vote_kernel": (new, 9 * Np * 4), "param_sign_step_kernel": (new, 2 * esz * n + Np * 4),
               "param_ef_kernel": (ef, (2 * esz + 4) * n)}
    for kernel, (fn, kb) in kernels.items():
        t, launches = P.kernel_time(fn, kernel, iters)
        if t:
            row.update({f"kernel_us_{kernel}": round(t, 2), f"kernel_launches_{kernel}": launches,
                        f"kernel_bytes_{kernel}": kb, f"kernel_tbps_{kernel}": round(kb / t / 1e6, 3)})
    row["new_vs_old"] = round(row["old_us"] / row["new_us"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--voters", type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the timer needs a ROCm device"
    with open(os.path.join(ROOT, "tests", "golden", "layouts.json")) as f:
        r50 = json.load(f)["resnet50_imagenet"]
    rows = []
    for name, dtype in (("resnet50_fp32", torch.float32), ("resnet50_bf16", torch.bfloat16)):
        rows.append(measure(name, r50, dtype, args.voters, args.iters, args.warmup, args.reps))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
