"""Time of the bucketed QSGD kernels (csrc/qsgd_bucket.hip) against the per-tensor QSGD path they
stand beside (csrc/qsgd.hip), in the same process, the windows alternating.

    python tools/qsgd_bucket_time.py [--out profiles/qsgd_bucket_time.json] [--iters 20] [--warmup 5] [--reps 5]

One JSON line per size (100M flat; ResNet-50's 25.6M), q = 4, B = 512.  Per pair, `new` against `base`:
  compress     qsgd_bucket_quant_kernel against qsgd_norm_kernel + qsgd_quant_kernel (x - x_hat)
  step         the fused-step kernel against choco_qsgd_recv_gossip_norms + choco_qsgd_compress, three
               pending messages (a ring); weights 0, no self message and gamma 0, so the buffers keep
               their values over the timed windows
  accumulate   the bucket accumulate against choco_qsgd_decompress_accumulate on a flat layout
               (accumulate_seg: the baseline on ResNet-50's per-tensor layout; the bucketed one has none)
  *_us / *_us_min_max    device time between two events per call (`iters` calls a window after `warmup`; the
               median over `reps` windows, min, max)
  *_kernel_us  the dispatch-attached time of the kernels alone (the library's profile hooks), summed per call
  *_bytes_per_element / *_tbps / *_of_peak   the traffic the path needs per element, and the rate that the
               kernel time makes of it against 8 TB/s
Needs a ROCm device; there is no fall-back.
"""
import argparse
import itertools
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

DEV, Q, B, NMSG, PEAK_TBPS = "cuda", 4, 512, 3, 8.0
MSG = Q / 8 + 1 / 8  # plane bytes per element; the scales add 4 / B (new) or nothing to speak of (base)
BYTES = {  # per element: reads + writes
    "compress_new": 8 + MSG + 4 / B, "compress_base": 16 + MSG,
    "step_new": 12 + NMSG * (MSG + 4 / B) + 8 + MSG + 4 / B, "step_base": 12 + NMSG * MSG + 8 + 8 + MSG,
    "accumulate_new": 4 + NMSG * (MSG + 4 / B) + 4, "accumulate_base": 4 + NMSG * MSG + 4,
    "accumulate_seg_base": 4 + NMSG * MSG + 4,
}
KERNELS = {"compress_new": ["qsgd_bucket_quantize"], "compress_base": ["qsgd_norm", "qsgd_quantize"],
           "step_new": ["qsgd_bucket_step"], "step_base": ["qsgd_recv_norm", "qsgd_quantize"],
           "accumulate_new": ["qsgd_bucket_accumulate"], "accumulate_base": ["qsgd_accumulate"],
           "accumulate_seg_base": ["qsgd_accumulate"]}


def ways(n, lens):
    g = torch.Generator(device=DEV).manual_seed(n)
    x, xh, mem = (torch.randn(n, generator=g, device=DEV) for _ in range(3))
    nseg = len(lens)
    seg_off = torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int64, device=DEV)
    new_msgs, base_msgs, seg_msgs = [], [], []
    for i in range(NMSG):
        d = torch.randn(n, generator=g, device=DEV)
        new_msgs.append(codec.qsgd_bucket_compress(d, Q, bucket=B, seed=i)[0])
        base_msgs.append(codec.qsgd_compress(d, Q, seed=i)[:2])
        seg_msgs.append(codec.qsgd_compress(d, Q, seg_off=seg_off, nseg=nseg, seed=i)[:2])
    out_new = codec.qsgd_bucket_wire(n, Q, B, DEV)
    _, out_base = codec.qsgd_wire(n, Q, 1, DEV)
    w = [0.0] * NMSG

    def step_base():
        codec.qsgd_recv_gossip_norms(base_msgs, w, -1, x, mem, xh, 0.0, Q, out=out_base[1])
        codec.qsgd_compress(x, Q, xhat=xh, norm_in=out_base[1], seed=1, out=out_base)

    return {
        "compress_new": lambda: codec.qsgd_bucket_compress(x, Q, bucket=B, xhat=xh, seed=1, out=out_new),
        "compress_base": lambda: codec.qsgd_compress(x, Q, xhat=xh, seed=1, out=out_base),
        "step_new": lambda: codec.qsgd_bucket_recv_gossip_compress(new_msgs, w, -1, x, mem, xh, 0.0, Q, bucket=B, seed=1,
                                                                   out=out_new),
        "step_base": step_base,
        "accumulate_new": lambda: codec.qsgd_bucket_accumulate(new_msgs, w, -1, n, Q, mem, bucket=B),
        "accumulate_base": lambda: codec.qsgd_accumulate(base_msgs, w, -1, n, Q, mem),
        "accumulate_seg_base": lambda: codec.qsgd_accumulate(seg_msgs, w, -1, n, Q, mem, seg_off=seg_off, nseg=nseg),
    }


def measure(name, lens, iters, warmup, reps):
    n = sum(lens)
    fns = ways(n, lens)
    for fn in fns.values():
        P.events(fn, warmup)
    runs = {tag: [] for tag in fns}
    for _ in range(reps):  # alternating windows: drift of the clocks lands on every way alike
        for tag, fn in fns.items():
            runs[tag].append(P.events(fn, iters)[1])
    row = {"layout": name, "elements": n, "q": Q, "bucket": B, "pending_messages": NMSG, "iters": iters,
           "warmup": warmup, "reps": reps}
    for tag, fn in fns.items():
        row[f"{tag}_us"] = round(statistics.median(runs[tag]), 1)
        row[f"{tag}_us_min_max"] = [round(min(runs[tag]), 1), round(max(runs[tag]), 1)]
        kus = sum(P.kernel_time(fn, k, iters)[0] or 0.0 for k in KERNELS[tag])
        row[f"{tag}_kernel_us"] = round(kus, 1)
        row[f"{tag}_bytes_per_element"] = round(BYTES[tag], 3)
        tbps = BYTES[tag] * n / kus / 1e6 if kus else None
        row[f"{tag}_tbps"], row[f"{tag}_of_peak"] = round(tbps, 3), round(tbps / PEAK_TBPS, 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qsgd_bucket_time.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qsgd_bucket_time needs a ROCm device")
    with open(os.path.join(ROOT, "tests", "golden", "layouts.json")) as f:
        resnet50 = json.load(f)["resnet50_imagenet"]
    rows = [measure("flat_100M", [100_000_000], a.iters, a.warmup, a.reps),
            measure("resnet50_fp32", resnet50, a.iters, a.warmup, a.reps)]
    with open(a.out, "w") as f:
        for row in rows:
            line = json.dumps(row)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
