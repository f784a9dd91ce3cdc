"""Golden-vector generator for DGC._apply_gradient with gradient clipping
(dl_code/pcode/optim/dgc.py:254-324).

Runs ONLY in the authoring container, where the upstream reference is mounted read-only at
/root/reference: it builds the reference's own optimizer with object.__new__ (as
gen_golden.gen_dgc does), runs _apply_gradient on CPU fp32 tensors and records inputs and
outputs as .npz fixtures next to this script.  Nothing from the reference is copied: the
fixtures are data only.

    dgc_sgd_inputs.npz    lens, p0, g0, g1, g2 (flat, the tensors back to back), clip_grad_val,
                          n_nodes, thr (the threshold in double, as _clip_gradient computes it)
    dgc_sgd_<set>.npz     hp = [lr, weight_decay, momentum, dampening, nesterov], and after each
                          of three consecutive steps k: d<k> (d_p, what p.grad.data holds),
                          buf<k> (momentum sets), norm<k> (the norm each _clip_gradient call saw,
                          one per tensor; the bound method is wrapped to record it)

_apply_gradient does not touch the parameters (DGC updates them in _recover_info), so p0 holds
for all three steps.  Every step gets a fresh gradient tensor.

Layout: 8195 crosses a tile with cut groups at both ends, 17000 spans three tiles, the two 40s
hold one inf and one NaN gradient, and the last tensor's one gradient equals (float)thr
exactly (its parameter is 0), so its norm is exact on every machine and pins the `>=`.

Usage:  python tests/golden/gen_golden_dgc_sgd.py
"""
import collections
import math
import os
import sys
import types

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference

import numpy as np  # noqa: E402
import torch  # noqa: E402

REF = "/root/reference/dl_code"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
# the reference's sparsification module imports the unvendored bit2byte packing extension, which
# nothing here calls: an empty module lets the import pass (gen_golden.py stubs it the same way)
sys.modules.setdefault("bit2byte", types.ModuleType("bit2byte"))

import pcode.optim.dgc as ref_dgc  # noqa: E402

LENS = [5, 1, 0, 8195, 33, 4099, 17000, 40, 40, 1]
SCALE = [0.01, 0.02, 1.0, 1.0, 0.01, 0.001, 1.0, 1.0, 1.0, 1.0]  # per-tensor gradient scale
N_NODES = 3
STEPS = 3
CLIP_VALS = [1.0, 2.0, 3.0, 5.0]  # the first whose (1 / thr) * thr != 1 in fp32 is kept
SETS = {  # lr, weight_decay, momentum, dampening, nesterov
    "clip": (0.1, 0.0, 0.0, 0.0, False),
    "wd": (0.05, 1e-4, 0.0, 0.0, False),
    "mom": (0.1, 1e-4, 0.9, 0.0, False),
    "nesterov": (0.1, 5e-4, 0.9, 0.0, True),
    "damp": (0.01, 1e-4, 0.9, 0.1, False),
}


def threshold(val):
    t = val
    t *= 1.0 / math.sqrt(N_NODES)  # dgc.py:262
    return t


def inputs(val):
    rng = np.random.RandomState(20240913)
    n = sum(LENS)
    offs = np.concatenate([[0], np.cumsum(LENS)])
    p0 = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32)
    gs = []
    for k in range(STEPS):
        g = rng.standard_normal(n).astype(np.float32)
        for s, sc in enumerate(SCALE):
            g[offs[s]:offs[s + 1]] *= np.float32(sc)
        g[offs[7] + 3 + k] = np.inf
        g[offs[8] + 11 + k] = np.nan
        g[offs[9]] = np.float32(threshold(val)) * np.float32(-1.0 if k == 1 else 1.0)
        g[offs[3] + 1], g[offs[3] + 2] = 0.0, -0.0
        gs.append(g)
    p0[offs[9]] = 0.0
    return p0, gs


def split(flat):
    out, o = [], 0
    for m in LENS:
        out.append(torch.from_numpy(flat[o:o + m].copy()))
        o += m
    return out


def cat(tensors):
    return np.concatenate([t.detach().numpy().reshape(-1) for t in tensors]).astype(np.float32)


def run(hp, val, p0, gs):
    lr, wd, mom, damp, nest = hp
    params = [torch.nn.Parameter(t) for t in split(p0)]
    opt = object.__new__(ref_dgc.DGC)
    opt.param_groups = [{"params": [p], "lr": lr, "weight_decay": wd, "momentum": mom, "dampening": damp,
                         "nesterov": nest} for p in params]
    opt.state = collections.defaultdict(dict)
    opt.clip_grad, opt.clip_grad_val, opt.n_nodes = True, val, N_NODES
    seen = []
    inner = opt._clip_gradient

    def recording(grad, param_state, scale=True):
        seen.append(float(grad.norm(p=2)))  # the value the call below computes and compares
        return inner(grad, param_state, scale)

    opt._clip_gradient = recording
    out = {"hp": np.array([lr, wd, mom, damp, float(nest)], dtype=np.float64)}
    for k in range(STEPS):
        del seen[:]
        for p, g in zip(params, split(gs[k])):
            p.grad = g
        opt._apply_gradient()
        assert len(seen) == len(LENS)
        out[f"norm{k}"] = np.array(seen, dtype=np.float32)
        assert np.array_equal(out[f"norm{k}"].astype(np.float64)[np.isfinite(seen)], np.array(seen)[np.isfinite(seen)])
        out[f"d{k}"] = cat([p.grad.data for p in params])
        if mom != 0:
            out[f"buf{k}"] = cat([opt.state[p]["momentum_buffer"] for p in params])
    assert np.array_equal(cat([p.data for p in params]).view(np.uint32), p0.view(np.uint32))
    return out


def checks(val, outs, gs):
    """What the tests rely on; False: try the next clip_grad_val."""
    thr = threshold(val)
    offs = np.concatenate([[0], np.cumsum(LENS)])
    for name, out in outs.items():
        for k in range(STEPS):
            nrm = out[f"norm{k}"].astype(np.float64)
            fin = [s for s in range(len(LENS) - 1) if np.isfinite(nrm[s]) and LENS[s] > 0]
            clipped = [s for s in fin if nrm[s] >= thr]
            if len(clipped) < 2 or len(fin) - len(clipped) < 2:
                return False
            if any(abs(nrm[s] - thr) <= 1e-3 * thr for s in fin):
                return False
            if nrm[-1] != np.float32(thr):
                return False
            if name == "clip":  # the pinned tensor is clipped, and clipping changes its bits
                if out[f"d{k}"][offs[9]] == gs[k][offs[9]]:
                    return False
    return True


def main():
    torch.set_num_threads(1)
    for val in CLIP_VALS:
        p0, gs = inputs(val)
        outs = {name: run(hp, val, p0, gs) for name, hp in SETS.items()}
        if checks(val, outs, gs):
            break
    else:
        raise SystemExit("no clip_grad_val of the list satisfies the fixture's conditions")
    print("clip_grad_val", val, "thr", threshold(val))
    np.savez_compressed(os.path.join(OUT, "dgc_sgd_inputs.npz"), lens=np.array(LENS, dtype=np.int64), p0=p0,
                        clip_grad_val=np.float64(val), n_nodes=np.int64(N_NODES), thr=np.float64(threshold(val)),
                        **{f"g{k}": g for k, g in enumerate(gs)})
    for name, out in outs.items():
        path = os.path.join(OUT, f"dgc_sgd_{name}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
