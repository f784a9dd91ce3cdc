"""Time of the MX (block-scaled FP4 / FP8) kernels (csrc/mx.hip) against bucketed QSGD at q = 4,
B = 512 (csrc/qsgd_bucket.hip), in the same process, the windows alternating.

    python tools/mx_time.py [--out profiles/mx_time.json] [--iters 20] [--warmup 5] [--reps 5]

One JSON line per size (100M flat; ResNet-50's 25.6M).  Ways: `bucket` (the baseline), and
`e2m1_sr`, `e2m1_rn`, `e4m3_sr`, `e4m3_rn` (format, stochastic / nearest-even rounding); per way
  compress     the one-pass compress of x - x_hat
  accumulate   three messages into memory
  step         the fused step with three pending messages (a ring); weights 0, no self message and
               gamma 0, so the buffers keep their values over the timed windows
  *_us / *_us_min_max    device time between two events per call (`iters` calls a window after `warmup`; the
               median over `reps` windows, min, max)
  *_kernel_us  the dispatch-attached time of the kernel alone (the library's profile hooks)
  *_bytes_per_element / *_of_peak   the traffic the path needs per element, and the rate that the kernel
               time makes of it against 8 TB/s
Needs a ROCm device; there is no fall-back.
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

DEV, B, NMSG, PEAK_TBPS = "cuda", 512, 3, 8.0
WAYS = {"bucket": (4, None), "e2m1_sr": (4, False), "e2m1_rn": (4, True), "e4m3_sr": (8, False), "e4m3_rn": (8, True)}


def wire_bytes(way):
    """message bytes per element"""
    q, biased = WAYS[way]
    return q / 8 + 1 / 8 + 4 / B if biased is None else q / 8 + 1 / 32


def traffic(op, way):
    m = wire_bytes(way)
    return {"compress": 8 + m, "accumulate": 8 + NMSG * m, "step": 12 + NMSG * m + 8 + m}[op]


def kernel(op, way):
    return ("qsgd_bucket_" if way == "bucket" else "mx_") + {"compress": "quantize", "accumulate": "accumulate",
                                                             "step": "step"}[op]


def calls(n):
    g = torch.Generator(device=DEV).manual_seed(n)
    x, xh, mem = (torch.randn(n, generator=g, device=DEV) for _ in range(3))
    deltas = [torch.randn(n, generator=g, device=DEV) for _ in range(NMSG)]
    w = [0.0] * NMSG
    fns = {}
    for way, (q, biased) in WAYS.items():
        if biased is None:
            msgs = [codec.qsgd_bucket_compress(d, q, bucket=B, seed=i)[0] for i, d in enumerate(deltas)]
            out = codec.qsgd_bucket_wire(n, q, B, DEV)
            fns["compress", way] = lambda q=q, out=out: codec.qsgd_bucket_compress(x, q, bucket=B, xhat=xh, seed=1, out=out)
            fns["accumulate", way] = lambda q=q, msgs=msgs: codec.qsgd_bucket_accumulate(msgs, w, -1, n, q, mem, bucket=B)
            fns["step", way] = lambda q=q, msgs=msgs, out=out: codec.qsgd_bucket_recv_gossip_compress(
                msgs, w, -1, x, mem, xh, 0.0, q, bucket=B, seed=1, out=out)
        else:
            msgs = [codec.mx_compress(d, q, is_biased=biased, seed=i)[0] for i, d in enumerate(deltas)]
            out = codec.mx_wire(n, q, DEV)
            kw = dict(is_biased=biased, seed=1, out=out)
            fns["compress", way] = lambda q=q, kw=kw: codec.mx_compress(x, q, xhat=xh, **kw)
            fns["accumulate", way] = lambda q=q, msgs=msgs: codec.mx_accumulate(msgs, w, -1, n, q, mem)
            fns["step", way] = lambda q=q, msgs=msgs, kw=kw: codec.mx_recv_gossip_compress(msgs, w, -1, x, mem, xh, 0.0,
                                                                                           q, **kw)
    return fns


def measure(name, n, iters, warmup, reps):
    fns = calls(n)
    for fn in fns.values():
        P.events(fn, warmup)
    runs = {tag: [] for tag in fns}
    for _ in range(reps):  # alternating windows: drift of the clocks lands on every way alike
        for tag, fn in fns.items():
            runs[tag].append(P.events(fn, iters)[1])
    row = {"layout": name, "elements": n, "bucket": B, "pending_messages": NMSG, "iters": iters, "warmup": warmup,
           "reps": reps}
    for (op, way), fn in fns.items():
        tag = f"{op}_{way}"
        row[f"{tag}_us"] = round(statistics.median(runs[op, way]), 1)
        row[f"{tag}_us_min_max"] = [round(min(runs[op, way]), 1), round(max(runs[op, way]), 1)]
        kus = P.kernel_time(fn, kernel(op, way), iters)[0] or 0.0
        row[f"{tag}_kernel_us"] = round(kus, 1)
        row[f"{tag}_bytes_per_element"] = round(traffic(op, way), 3)
        row[f"{tag}_of_peak"] = round(traffic(op, way) * n / kus / 1e6 / PEAK_TBPS, 3) if kus else None
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_time.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mx_time needs a ROCm device")
    with open(os.path.join(ROOT, "tests", "golden", "layouts.json")) as f:
        resnet50 = sum(json.load(f)["resnet50_imagenet"])
    rows = [measure("flat_100M", 100_000_000, a.iters, a.warmup, a.reps),
            measure("resnet50_fp32", resnet50, a.iters, a.warmup, a.reps)]
    with open(a.out, "w") as f:
        for row in rows:
            line = json.dumps(row)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
