"""numpy model of the three kernels of DGC's optimizer half (include/choco_codec.h:
choco_params_sqnorm, choco_params_sgd_clip, choco_params_mask; dl_code/pcode/optim/dgc.py:
254-324 and :174-182).  Values of 16-bit tensors are fp32 arrays on the dtype's grid, as in
_sgd_oracle, whose fma32 / to_grid this imports.

    d = g
    if wd  != 0:  d = fma(wd, p, d)
    if norm given:  c = norm >= (float)thr ? (1 / norm) * (float)thr : 1;  d = c * d
    if mom != 0:  ... as _sgd_oracle.sgd_step ...
"""
import numpy as np

from _sgd_oracle import F32, fma32, mul32, scalars, to_grid


def decayed(p, g, wd, dtype="fp32"):
    """The d the norm is taken of and the clip scales: g, or fma(wd, p, g)."""
    d = np.asarray(g, F32)
    if wd != 0:
        d = to_grid(fma32(F32(wd), np.asarray(p, F32), d), dtype)
    return d


def sqnorm(p, g, wd=0.0, dtype="fp32"):
    """float32(sqrt(sum(d^2))) with squares and sum in float64, narrowed to the dtype's grid."""
    d = decayed(p, g, wd, dtype).astype(np.float64)
    with np.errstate(all="ignore"):
        r = F32(np.sqrt(np.sum(d * d))) if d.size else F32(0)
    return to_grid(np.array([r], F32), dtype)[0]


def clip_coef(norm, thr):
    """torch's `threshold / grad_norm` behind an fp32 comparison: reciprocal, then multiply."""
    norm, thr = F32(norm), F32(thr)
    with np.errstate(all="ignore"):
        return F32(F32(1) / norm) * thr if norm >= thr else F32(1)


def sgd_step(p, g, buf, lr, wd=0.0, mom=0.0, damp=0.0, nesterov=False, first=False, dtype="fp32", norm=None,
             thr=None):
    """One update of one tensor.  Returns (p_new, buf_new or None, d_p) like _sgd_oracle.sgd_step;
    norm / thr None: no clipping."""
    nlr, wdf, momf, omd = scalars(lr, wd, mom, damp)
    p = np.asarray(p, F32)
    d = decayed(p, g, wd, dtype)
    if norm is not None:
        d = to_grid(mul32(clip_coef(norm, thr), d), dtype)
    buf_new = None
    if mom != 0:
        if first:
            buf_new = to_grid(fma32(F32(1), d, mul32(F32(0), momf)), dtype)
        else:
            t = to_grid(mul32(buf, momf), dtype)
            buf_new = to_grid(fma32(omd, d, t), dtype)
        d = to_grid(fma32(momf, buf_new, d), dtype) if nesterov else buf_new
    return to_grid(fma32(nlr, d, p), dtype), buf_new, d


def split(flat, lens):
    out, o = [], 0
    for m in lens:
        out.append(np.asarray(flat[o:o + m]))
        o += m
    return out


def step_layout(p, g, buf, lens, hp, first, norms=None, thr=None, dtype="fp32"):
    """sgd_step over a flat layout.  Returns flat (p_new, buf_new or None, d_p)."""
    lr, wd, mom, damp, nest = hp
    ps, gs = split(p, lens), split(g, lens)
    bs = split(buf, lens) if buf is not None else [None] * len(lens)
    outs = [sgd_step(ps[s], gs[s], bs[s], lr, wd, mom, damp, nest, first, dtype,
                     None if norms is None else norms[s], thr) for s in range(len(lens))]
    cat = lambda i: np.concatenate([np.asarray(o[i], F32).reshape(-1) for o in outs]).astype(F32)  # noqa: E731
    return cat(0), (cat(1) if mom != 0 else None), cat(2)


def norms_layout(p, g, lens, wd, dtype="fp32"):
    return np.array([sqnorm(a, b, wd, dtype) for a, b in zip(split(p, lens), split(g, lens))], F32)


def mask(bufs, dtypes, lens, values, indices, k_per_seg, memory=None):
    """choco_params_mask: bufs (list of fp32 arrays on their dtype's grid, or None) and memory are
    updated in place.  An index outside its tensor's flat range is skipped."""
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    j = 0
    with np.errstate(all="ignore"):
        for s, ks in enumerate(k_per_seg):
            for jj in range(j, j + int(ks)):
                i = int(indices[jj])
                if not (offs[s] <= i < offs[s + 1]):
                    continue
                if bufs[s] is not None:
                    e = i - int(offs[s])
                    bufs[s][e] = to_grid(mul32(bufs[s][e], F32(0)), dtypes[s]).reshape(-1)[0]
                if memory is not None:
                    v = F32(values[jj])
                    memory[i] = v + (-v)
            j += int(ks)
