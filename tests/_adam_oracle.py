"""numpy restatement of the per-element Adam / AdamW update of choco_params_adam and
choco_params_adam_master (include/choco_codec.h), on tests/_sgd_oracle.py's fma32 / mul32 /
to_grid.  The hyperparameters are computed in Python doubles exactly as
torch.optim.adam._single_tensor_adam computes them and narrowed once to fp32; `step` is the
count after the increment:

    bc1 = 1 - beta1**step;  bc2 = 1 - beta2**step
    nss = f32(-(lr / bc1));  bs = f32(bc2 ** 0.5);  dec = f32(1 - lr * wd)
    w = f32(1 - beta1);  b2 = f32(beta2);  omb2 = f32(1 - beta2);  e = f32(eps)

Per element, each line one rounding (rnd: identity in fp32, the round-to-nearest-even narrowing
to the tensor's grid for bf16 / fp16):

    g' = g                                    (coef c given: g' = rnd(c * g))
    if wd != 0:  decoupled:  p  = rnd(p * dec)
                 coupled:    g' = rnd(fma(wd, p, g'))
    d = g' - m                                (fp32, not narrowed)
    m = w < 0.5 ? rnd(fma(w, d, m)) : rnd(fma(-(1 - w), d, g'))
    v = rnd(v * b2);  t = omb2 * g';  v = rnd(fma(t, g', v))
    den = rnd(sqrt(v));  den = rnd(den / bs);  den = rnd(den + e)
    q = m / den;  p_new = rnd(fma(nss, q, p))

first: the tensor has no state yet, m = v = +0 whatever is passed.  A skipped op (wd == 0) is
skipped.  The master side (adam_master_step) is the fp32 lines on the fp32 master copy with the
widened gradient, fp32 moments and an unnarrowed coefficient product; the 16-bit parameter is
the new master value narrowed once.
"""
import numpy as np

from _sgd_oracle import F32, fma32, mul32, to_grid


def scalars(lr, beta1, beta2, eps, wd, step):
    """(nss, bs, dec, w, b2, omb2, e, wdf), each a Python double narrowed once to fp32."""
    step = float(step)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    return (F32(-(lr / bc1)), F32(bc2 ** 0.5), F32(1 - lr * wd), F32(1 - beta1), F32(beta2), F32(1 - beta2),
            F32(eps), F32(wd))


def _f32(op, a, b):
    with np.errstate(all="ignore"):
        return op(np.asarray(a, F32), np.asarray(b, F32)).astype(F32)


def adam_step(p, g, m, v, lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, step=1, decoupled=False, first=False,
              coef=None, dtype="fp32", narrow_coef=True):
    """One update.  Returns (p_new, m_new, v_new, g') as fp32 arrays on the dtype's grid (g' is
    the gradient the lines took after the coefficient: what WRITE_CLIPPED stores, narrowed)."""
    nss, bs, dec, w, b2, omb2, e, wdf = scalars(lr, beta1, beta2, eps, wd, step)
    p, gp = np.asarray(p, F32), np.asarray(g, F32)
    if first:
        m, v = np.zeros_like(p), np.zeros_like(p)
    m, v = np.asarray(m, F32), np.asarray(v, F32)
    if coef is not None:
        gp = mul32(F32(coef), gp)
        if narrow_coef:
            gp = to_grid(gp, dtype)
    clipped = gp
    if wd != 0:
        if decoupled:
            p = to_grid(mul32(p, dec), dtype)
        else:
            gp = to_grid(fma32(wdf, p, gp), dtype)
    d = _f32(np.subtract, gp, m)
    if w < F32(0.5):
        m = to_grid(fma32(w, d, m), dtype)
    else:
        m = to_grid(fma32(-(F32(1) - w), d, gp), dtype)
    v = to_grid(mul32(v, b2), dtype)
    t = mul32(omb2, gp)
    v = to_grid(fma32(t, gp, v), dtype)
    with np.errstate(all="ignore"):
        den = to_grid(np.sqrt(v).astype(F32), dtype)
    den = to_grid(_f32(np.divide, den, bs), dtype)
    den = to_grid(_f32(np.add, den, e), dtype)
    q = _f32(np.divide, m, den)
    return to_grid(fma32(nss, q, p), dtype), m, v, clipped


def adam_master_step(master, g, m, v, lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, step=1, decoupled=False,
                     first=False, coef=None, dtype="fp32"):
    """One update on the master copy.  master, m, v: fp32 arrays; g: fp32 array on `dtype`'s
    grid (the widened gradient).  Returns (master_new, m_new, v_new, the parameter on its
    dtype's grid, the clipped gradient narrowed to the grid)."""
    p_new, m_new, v_new, gc = adam_step(master, g, m, v, lr, beta1, beta2, eps, wd, step, decoupled, first, coef,
                                        dtype="fp32", narrow_coef=False)
    return p_new, m_new, v_new, to_grid(p_new, dtype), to_grid(gc, dtype)
