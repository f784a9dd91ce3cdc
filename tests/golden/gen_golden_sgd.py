"""Golden-vector generator for apply_gradient (dl_code/pcode/optim/utils.py:13-47).

Runs ONLY in the authoring container, where the upstream reference is mounted read-only at
/root/reference: it imports the reference's own apply_gradient, as gen_golden.py imports the
compressors, runs it on CPU fp32 tensors and records inputs and outputs as .npz fixtures next
to this script.  Nothing from the reference is copied: the fixtures are data only.

    sgd_inputs.npz           lens, p0, g0, g1, g2 (flat, the tensors back to back)
    sgd_<set>_<mode>.npz     hp = [lr, weight_decay, momentum, dampening, nesterov], and after
                             each of three consecutive steps k: p<k>, buf<k> (momentum sets),
                             d<k> (d_p) -- all flat

<mode>: apply (apply_grad_to_model=True) or grad (False).  d_p is recorded where the reference
leaves it observable: p.grad.data after the call in grad mode and, in apply mode, without
momentum (the in-place weight decay); with momentum and no Nesterov it is the buffer (not
stored twice), and the Nesterov d_p of apply mode is a temporary (p pins it).  Every step gets
a fresh gradient tensor, so the reference's rebinding of p.grad to the buffer never aliases the
next step's gradient.

Usage:  python tests/golden/gen_golden_sgd.py
"""
import collections
import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference

import numpy as np  # noqa: E402
import torch  # noqa: E402

REF = "/root/reference/dl_code"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

import pcode.optim.utils as ref_ou  # noqa: E402

LENS = [5, 1, 0, 8195, 33, 4099]
STEPS = 3
SETS = {  # lr, weight_decay, momentum, dampening, nesterov
    "plain": (0.1, 0.0, 0.0, 0.0, False),
    "wd": (0.05, 1e-4, 0.0, 0.0, False),
    "mom": (0.1, 0.0, 0.9, 0.0, False),
    "nesterov": (0.1, 5e-4, 0.9, 0.0, True),
    "damp": (0.01, 1e-4, 0.9, 0.1, False),
}


def inputs():
    rng = np.random.RandomState(20240607)
    n = sum(LENS)
    p0 = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32)
    gs = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n)).astype(np.float32) for _ in range(STEPS)]
    sub = np.float32(1e-41)
    special = [0.0, -0.0, np.inf, -np.inf, np.nan, sub, -sub, 1e-38]
    # specials in p against ordinary g, in g against ordinary p, and against each other
    base = LENS[0] + LENS[1] + 100
    for i, v in enumerate(special):
        p0[base + i] = v
        for k, g in enumerate(gs):
            g[base + 20 + i] = v
            g[base + 40 + i] = special[(i + k + 1) % len(special)]
        p0[base + 40 + i] = v
    p0[0], gs[0][0], gs[1][0] = -0.0, -0.0, 0.0
    p0[1], gs[0][1] = 0.0, -0.0
    return p0, gs


def split(flat):
    out, o = [], 0
    for m in LENS:
        out.append(torch.from_numpy(flat[o:o + m].copy()))
        o += m
    return out


def cat(tensors):
    return np.concatenate([t.detach().numpy().reshape(-1) for t in tensors]).astype(np.float32)


def run(hp, apply_mode, p0, gs):
    lr, wd, mom, damp, nest = hp
    params = [torch.nn.Parameter(t) for t in split(p0)]
    groups = [{"params": [p], "lr": lr, "weight_decay": wd, "momentum": mom, "dampening": damp, "nesterov": nest}
              for p in params]
    state = collections.defaultdict(dict)
    out = {"hp": np.array([lr, wd, mom, damp, float(nest)], dtype=np.float64)}
    for k in range(STEPS):
        for p, g in zip(params, split(gs[k])):
            p.grad = g
        ref_ou.apply_gradient(groups, state, apply_grad_to_model=apply_mode)
        out[f"p{k}"] = cat([p.data for p in params])
        if mom != 0:
            out[f"buf{k}"] = cat([state[p]["momentum_buffer"] for p in params])
        if not apply_mode or mom == 0:
            out[f"d{k}"] = cat([p.grad.data for p in params])
    return out


def main():
    p0, gs = inputs()
    np.savez_compressed(os.path.join(OUT, "sgd_inputs.npz"), lens=np.array(LENS, dtype=np.int64), p0=p0,
                        **{f"g{k}": g for k, g in enumerate(gs)})
    for name, hp in SETS.items():
        for apply_mode in (True, False):
            path = os.path.join(OUT, f"sgd_{name}_{'apply' if apply_mode else 'grad'}.npz")
            np.savez_compressed(path, **run(hp, apply_mode, p0, gs))
            print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
