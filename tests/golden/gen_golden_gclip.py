"""Golden-vector generator for global-norm gradient clipping in front of apply_gradient: the
language-model loop's torch.nn.utils.clip_grad_norm_(model.parameters(), conf.rnn_clip) followed
by optimizer.step (dl_code/pcode/distributed_running_nlp.py:94-97, dl_code/pcode/optim/utils.py:13-47).

Runs ONLY in the authoring container, where the upstream reference is mounted read-only at
/root/reference: it imports the reference's own apply_gradient, as gen_golden_sgd.py does, runs
the real sequence on CPU fp32 tensors and records inputs and outputs as .npz fixtures next to
this script.  Nothing from the reference is copied: the fixtures are data only.

    gclip_inputs.npz    lens, p0, g0, g1, g2 (flat, the tensors back to back), max_norm, and the
                        one-element case: one_p0, one_g, one_max_norm, one_lr, one_total, one_gc,
                        one_p (g = 1.0 and max_norm = 1.0: the total is exact on every machine
                        and the gradient is still scaled -- there is no `>=` shortcut)
    gclip_<set>.npz     hp = [lr, weight_decay, momentum, dampening, nesterov], and after each of
                        three consecutive steps k: total<k> (what clip_grad_norm_ returned),
                        gc<k> (the clipped gradients, copied before apply_gradient adds the
                        weight decay into them), p<k>, buf<k> (momentum sets) -- all flat

Layout: a zero-length tensor, 8195 crosses a tile with cut groups at both ends, 17000 spans
three tiles, 1500 is a whole-workgroup span inside a tile.  The gradient scale falls from step
to step so that, with the one max_norm, step 0 is clipped (c < 1) and step 2 is not (c == 1).

Usage:  python tests/golden/gen_golden_gclip.py
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

LENS = [5, 1, 0, 8195, 33, 4099, 17000, 40, 1500, 1]
STEPS = 3
MAX_NORM = 0.4                      # exps/finetune-lstm/example.sh
STEP_SCALE = [1.0, 0.01, 1e-4]      # totals of about 175, 1.75 and 0.0175
SETS = {  # lr, weight_decay, momentum, dampening, nesterov
    "clip": (0.1, 0.0, 0.0, 0.0, False),
    "wd": (0.05, 1e-4, 0.0, 0.0, False),
    "mom": (0.1, 1e-4, 0.9, 0.0, False),
    "nesterov": (0.1, 5e-4, 0.9, 0.0, True),
    "damp": (0.01, 1e-4, 0.9, 0.1, False),
}


def inputs():
    rng = np.random.RandomState(20241020)
    n = sum(LENS)
    offs = np.concatenate([[0], np.cumsum(LENS)])
    p0 = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32)
    gs = []
    for k in range(STEPS):
        g = (rng.standard_normal(n) * STEP_SCALE[k]).astype(np.float32)
        g[offs[3] + 1], g[offs[3] + 2] = 0.0, -0.0
        gs.append(g)
    return p0, gs


def split(flat, lens=LENS):
    out, o = [], 0
    for m in lens:
        out.append(torch.from_numpy(flat[o:o + m].copy()))
        o += m
    return out


def cat(tensors):
    return np.concatenate([t.detach().numpy().reshape(-1) for t in tensors]).astype(np.float32)


def run(hp, max_norm, p0, gs, lens=LENS):
    lr, wd, mom, damp, nest = hp
    params = [torch.nn.Parameter(t) for t in split(p0, lens)]
    groups = [{"params": [p], "lr": lr, "weight_decay": wd, "momentum": mom, "dampening": damp, "nesterov": nest}
              for p in params]
    state = collections.defaultdict(dict)
    out = {"hp": np.array([lr, wd, mom, damp, float(nest)], dtype=np.float64)}
    for k, g in enumerate(gs):
        for p, t in zip(params, split(g, lens)):
            p.grad = t
        total = torch.nn.utils.clip_grad_norm_(params, max_norm)
        assert total.dtype == torch.float32 and total.dim() == 0
        out[f"total{k}"] = total.numpy().astype(np.float32).reshape(())
        out[f"gc{k}"] = cat([p.grad.data for p in params])
        ref_ou.apply_gradient(groups, state, apply_grad_to_model=True)
        out[f"p{k}"] = cat([p.data for p in params])
        if mom != 0:
            out[f"buf{k}"] = cat([state[p]["momentum_buffer"] for p in params])
    return out


def checks(outs, gs):
    """What the tests rely on."""
    for out in outs.values():
        assert float(out["total0"]) > 10 * MAX_NORM and float(out["total2"]) < 0.1 * MAX_NORM
        assert not np.array_equal(out["gc0"], gs[0]), "step 0 must be clipped"
        assert np.array_equal(out["gc2"].view(np.uint32), gs[2].view(np.uint32)), "step 2 must not be clipped"


def main():
    torch.set_num_threads(1)
    p0, gs = inputs()
    outs = {name: run(hp, MAX_NORM, p0, gs) for name, hp in SETS.items()}
    checks(outs, gs)
    one_p0, one_g, one_lr = np.array([0.5], np.float32), np.array([1.0], np.float32), 0.1
    one = run((one_lr, 0.0, 0.0, 0.0, False), 1.0, one_p0, [one_g], lens=[1])
    assert float(one["total0"]) == 1.0 and float(one["gc0"][0]) < 1.0, "the one-element case must be scaled"
    np.savez_compressed(os.path.join(OUT, "gclip_inputs.npz"), lens=np.array(LENS, dtype=np.int64), p0=p0,
                        max_norm=np.float64(MAX_NORM), one_p0=one_p0, one_g=one_g, one_max_norm=np.float64(1.0),
                        one_lr=np.float64(one_lr), one_total=one["total0"], one_gc=one["gc0"], one_p=one["p0"],
                        **{f"g{k}": g for k, g in enumerate(gs)})
    for name, out in outs.items():
        path = os.path.join(OUT, f"gclip_{name}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), [float(out[f"total{k}"]) for k in range(STEPS)])


if __name__ == "__main__":
    main()
