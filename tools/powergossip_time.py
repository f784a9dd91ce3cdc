"""Time of PowerGossip's five launches (csrc/lowrank_gossip.hip) on ResNet-50's layout for a ring worker
(E = 2 neighbours), against utils.dpsgd_step's device time on the same layout in the same process.

    python tools/powergossip_time.py [--out profiles/powergossip_time.json] [--iters 20] [--warmup 5] [--reps 5]

One JSON line per rank r in 1, 2, 4 (K = E r = 2, 4, 8), the peers' messages prepared buffers (no exchange):
  launches_us / dpsgd_us   device time between two events per call of the five launches (project, orthogonalise,
             back-project with the slab sum, diff, apply) and of utils.dpsgd_step with a loopback aggregator
             (`iters` calls a window after `warmup`, the two alternating; the median over `reps` windows, min, max)
  kernel_us_*    the dispatch-attached time of each kernel alone (the library's profile hooks)
  bytes_* / tbps_*   the three passes over X move 4 + 4 + 8 B per element (project and back-project read it, apply
             reads and writes it; back-project reads the compressed elements only), and the rate reached
  sent_bytes / dpsgd_sent_bytes   per worker per step: 4 E (msg1_len + msg2_len) against 4 E n
  ab_*       r = 4 only: each pass over X as ONE K = 8 launch against TWO K = 4 launches (one edge each)
With --wide, the wide family (csrc/lowrank_gossip_mfma.hip) instead, one JSON line per (E, r) of a 2 x 4 torus
(4, 4), a complete graph of 8 (7, 2), (7, 4) and a ring at ranks 8 and 16 (2, 8), (2, 16), and the narrow family
at (2, 4) for scale:
  launches_us, kernel_us_*, bytes_*, tbps_*   as above
  floor_us_* / roofline_*   the least time of a pass, the larger of bytes / 8 TB/s and 2 KW flop per element over
             the fp32 matrix peak (157.3 TFLOP/s), and that over the kernel's time
  fused_step_us / step_loop_us   device time between events of powergossip.fused_step and of powergossip.step_loop
             on the device (what fused_step ran for this (E, r) before the wide family), two models in one process,
             the windows alternating, prepared peer messages
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
from powersgd_time import resnet50_shapes  # noqa: E402
from chocosgd_amd import codec, powergossip, utils  # noqa: E402

E, DEV = 2, "cuda"
PASSES = {"lowrank_gossip_project_kernel": 4, "lowrank_gossip_backproject_kernel": 4, "lowrank_gossip_apply_kernel": 8}
OTHERS = ["lowrank_gossip_orth_kernel", "lowrank_gossip_slabsum_kernel", "lowrank_gossip_diff_kernel"]
WIDE_CASES = [(2, 4), (4, 4), (7, 2), (7, 4), (2, 8), (2, 16)]  # (E, r); the first is the narrow family's
WIDE_PASSES = {"lowrank_gossip_project_mfma_kernel": 4, "lowrank_gossip_backproject_mfma_kernel": 4,
               "lowrank_gossip_apply_mfma_kernel": 8}
PEAK_TBPS, PEAK_MATRIX_TFLOPS = 8.0, 157.3


class _Ring:
    """dpsgd_step's exchange for worker 1 of a ring: its own buffer and two prepared peers."""
    rank = 1

    def __init__(self, n):
        self.peers = {j: torch.randn(n, device=DEV) for j in (0, 2)}

    def _agg(self, data, op=None, **kw):
        return {0: self.peers[0], 1: data, 2: self.peers[2]}


def buffers(plan, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(plan.rank)
    n_e = plan.n_edges
    sizes = dict(x=plan.n, q=n_e * plan.msg2_len, msg1=n_e * plan.msg1_len, recv1=n_e * plan.msg1_len, phat=n_e * plan.p_total,
                 msg2=n_e * plan.msg2_len, recv2=n_e * plan.msg2_len, dq=n_e * plan.msg2_len)
    return {k: scale * torch.randn(m, generator=g, device=DEV) for k, m in sizes.items()}


def five(plan, b, mask, w):
    def run():
        plan.project(b["x"], b["q"], b["msg1"])
        plan.orthogonalize(b["msg1"], b["recv1"], b["phat"], mask)
        plan.backproject(b["x"], b["phat"], b["msg2"])
        plan.diff(b["msg2"], b["recv2"], b["q"], b["dq"], mask)
        plan.apply(b["x"], b["phat"], b["dq"], b["recv1"], w, mask)
    return run


def measure(shapes, r, iters, warmup, reps):
    plan = codec.LowRankGossipPlan(shapes, r, E, DEV)
    b = buffers(plan)
    _, groups, names = P.model(shapes, torch.float32)
    state, ring = collections.defaultdict(dict), _Ring(plan.n)
    info = {0: 1.0 / 3, 1: 1.0 / 3, 2: 1.0 / 3}
    # the low end of both edges: x <- x - w P^ (P^T x - ..) contracts, so x stays bounded over the timed windows
    ways = {"launches": five(plan, b, 0b11, [1.0 / 3] * E),
            "dpsgd": lambda: utils.dpsgd_step(groups, names, state, ring, info)}
    for fn in ways.values():
        P.events(fn, warmup)
    t = plan.table
    n_comp = sum(m for m, c in zip(t.lens, t.compressed) if c)
    row = {"layout": "resnet50_fp32", "rank": r, "edges": E, "elements": plan.n, "compressed_elements": n_comp,
           "sent_bytes": 4 * E * (plan.msg1_len + plan.msg2_len), "dpsgd_sent_bytes": 4 * E * plan.n,
           "iters": iters, "warmup": warmup, "reps": reps}
    runs = {tag: [] for tag in ways}
    for _ in range(reps):
        for tag, fn in ways.items():
            runs[tag].append(P.events(fn, iters)[1])
    for tag in ways:
        row[f"{tag}_us"] = round(statistics.median(runs[tag]), 1)
        row[f"{tag}_us_min_max"] = [round(min(runs[tag]), 1), round(max(runs[tag]), 1)]
    total = 0.0
    for kernel in list(PASSES) + OTHERS:
        us, launches = P.kernel_time(ways["launches"], kernel, iters)
        if not us:
            continue
        total += us
        row[f"kernel_us_{kernel}"], row[f"kernel_launches_{kernel}"] = round(us, 2), launches
        if kernel in PASSES:
            nbytes = PASSES[kernel] * (n_comp if "backproject" in kernel else plan.n)
            row[f"bytes_{kernel}"], row[f"tbps_{kernel}"] = nbytes, round(nbytes / us / 1e6, 3)
    row["kernel_us_launches"] = round(total, 2)
    if E * r == 8:  # one K = 8 pass against two K = 4 passes, one edge each
        one = codec.LowRankGossipPlan(shapes, r, 1, DEV)
        halves = [buffers(one) for _ in range(E)]
        calls = {"project": (lambda p, c: p.project(c["x"], c["q"], c["msg1"])),
                 "backproject": (lambda p, c: p.backproject(c["x"], c["phat"], c["msg2"])),
                 "apply": (lambda p, c: p.apply(b["x"] if p is plan else halves[0]["x"], c["phat"], c["dq"], c["recv1"],
                                                [0.0] * p.n_edges, 0))}  # zero weights: x stays as it is
        for name, call in calls.items():
            both = P.kernel_time(lambda: call(plan, b), f"lowrank_gossip_{name}_kernel", iters)[0]
            split = P.kernel_time(lambda: [call(one, h) for h in halves], f"lowrank_gossip_{name}_kernel", iters)[0]
            row[f"ab_{name}_k8_us"], row[f"ab_{name}_2xk4_us"] = round(both, 2), round(split, 2)
    return row


class _Peers:
    """fused_step's and step_loop's exchange for worker 1: prepared peer messages, drawn once per length."""
    rank = 1

    def __init__(self):
        self.got = {}

    def exchange_edges(self, messages, out=None):
        for j, t in messages.items():
            if (j, t.numel()) not in self.got:
                self.got[j, t.numel()] = torch.randn(t.numel(), device=DEV)
        got = {j: self.got[j, t.numel()] for j, t in messages.items()}
        return got if out is None else {j: out[j].copy_(t) for j, t in got.items()}


def measure_wide(shapes, E, r, iters, warmup, reps):
    cls = powergossip.plan_class(r, E)
    plan = cls(shapes, r, E, DEV)
    passes = WIDE_PASSES if cls is codec.LowRankGossipWidePlan else PASSES
    b = buffers(plan)
    # the low end of every edge, weights summing under 1: x stays bounded over the timed windows
    launches = five(plan, b, (1 << E) - 1, [1.0 / (E + 1)] * E)
    info = {j: 1.0 / (E + 1) for j in range(E + 1)}
    steps = {}
    for tag, fn in (("fused_step", powergossip.fused_step), ("step_loop", powergossip.step_loop)):
        _, groups, names = P.model(shapes, torch.float32)
        comp, state = powergossip.PowerGossipCompressor(r, _Peers(), info, seed=1), collections.defaultdict(dict)
        steps[tag] = lambda fn=fn, comp=comp, groups=groups, names=names, state=state: fn(comp, groups, names, state)
    loop_iters = max(2, iters // 5)  # a step_loop call is hundreds of launches
    ways = {"launches": (launches, iters), "fused_step": (steps["fused_step"], iters), "step_loop": (steps["step_loop"], loop_iters)}
    for fn, _ in ways.values():
        P.events(fn, min(warmup, 2))
    t = plan.table
    n_comp = sum(m for m, c in zip(t.lens, t.compressed) if c)
    KW = 16 if E * r <= 16 else 32
    row = {"layout": "resnet50_fp32", "family": cls.__name__, "rank": r, "edges": E, "width": E * r, "elements": plan.n,
           "compressed_elements": n_comp, "sent_bytes": 4 * E * (plan.msg1_len + plan.msg2_len), "iters": iters,
           "step_loop_iters": loop_iters, "reps": reps}
    runs = {tag: [] for tag in ways}
    for _ in range(reps):
        for tag, (fn, k) in ways.items():
            runs[tag].append(P.events(fn, k)[1])
    for tag in ways:
        row[f"{tag}_us"] = round(statistics.median(runs[tag]), 1)
        row[f"{tag}_us_min_max"] = [round(min(runs[tag]), 1), round(max(runs[tag]), 1)]
    total = 0.0
    for kernel in list(passes) + OTHERS:
        us, count = P.kernel_time(launches, kernel, iters)
        if not us:
            continue
        total += us
        row[f"kernel_us_{kernel}"], row[f"kernel_launches_{kernel}"] = round(us, 2), count
        if kernel in passes:
            elems = n_comp if "backproject" in kernel else plan.n
            nbytes = passes[kernel] * elems
            row[f"bytes_{kernel}"], row[f"tbps_{kernel}"] = nbytes, round(nbytes / us / 1e6, 3)
            if passes is WIDE_PASSES:
                floor = max(nbytes / PEAK_TBPS / 1e6, 2 * KW * n_comp / PEAK_MATRIX_TFLOPS / 1e6)
                row[f"floor_us_{kernel}"], row[f"roofline_{kernel}"] = round(floor, 2), round(floor / us, 3)
    row["kernel_us_launches"] = round(total, 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "powergossip_time.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--wide", action="store_true", help="the wide family's cases instead of the ring at ranks 1, 2, 4")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the timer needs a ROCm device"
    shapes = resnet50_shapes()
    rows = []
    for case in (WIDE_CASES if args.wide else (1, 2, 4)):
        rows.append(measure_wide(shapes, *case, args.iters, args.warmup, args.reps) if args.wide
                    else measure(shapes, case, args.iters, args.warmup, args.reps))
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
