"""Warm-path state of the segmented top-k after a few calls (csrc/topk_seg.hip): per
multi-tile segment the mode the last warm call took (0 select, 1 / 3 window missed below /
above -> shared exact select, 2 every element), its window and drift words, and the host's
warm / cold bookkeeping.  Read through codec.seg_windows / seg_info / seg_host_state
(include/choco_codec.h CHOCO_SEG_*).  python tools/seg_windows.py [--layout resnet50_imagenet]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chocosgd_amd import _lib, codec  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", default="resnet50_imagenet")
    ap.add_argument("--calls", type=int, default=6)
    a = ap.parse_args()
    with open(os.path.join(ROOT, "tests", "golden", "layouts.json")) as f:
        lens = json.load(f)[a.layout]
    dev = torch.device("cuda", 0)
    plan = codec.SegmentPlan(lens, 0.99, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    ds = [torch.randn(sum(lens), generator=g, device=dev) for _ in range(4)]
    for i in range(a.calls):
        codec.topk_segmented(ds[i % 4], plan)
    win = codec.seg_windows(plan)   # (synchronises)
    info = codec.seg_info(plan)
    multi = np.nonzero(win[:, codec.SEG_WIN_WORDS.index("valid")])[0]
    modes = info[multi, _lib.SEG_INFO_MODE]
    print(f"{plan.nseg} segments, {multi.size} with a window; modes of the last warm call: "
          f"select {int((modes == 0).sum())} missed {int(((modes == 1) | (modes == 3)).sum())} "
          f"all {int((modes == 2).sum())}")
    col = {w: i for i, w in enumerate(codec.SEG_WIN_WORDS)}
    for s in multi[(modes == 1) | (modes == 3)][:20]:
        print(f"  missed seg {s}: len {lens[s]} k {plan.k_per_seg[s]} used lo {info[s, _lib.SEG_INFO_LO]:#x} "
              f"sh {info[s, _lib.SEG_INFO_SH]}, next lo {win[s, col['lo']]:#x} sh {win[s, col['sh']]}")
    print("window sh histogram:", np.bincount(win[multi, col["sh"]], minlength=10).tolist())
    print("trust histogram:", np.bincount(win[multi, col["trust"]], minlength=16).tolist())
    print("host:", codec.seg_host_state(plan), "shadow (misses, checks):", codec.seg_shadow(plan))


if __name__ == "__main__":
    main()
