"""numpy restatement of the per-element arithmetic of choco_params_ef and
choco_sign_local_residual (include/choco_codec.h), each line one fp32 op with one rounding:

    accum:     flat = flat + x                          deep_squeeze.py:101-108
    apply:     a = flat
        div:     a = a / (float)divisor, flat = a       ef_sign_sgd.py:218 (true division)
        scale:   a = (float)(-lr) * a                   ef_sign_sgd.py:119
               params = (x + a) narrowed to the dtype's grid, once
    residual:  u = (norm_s * sign(x)) / numel_s, resid = x - u      sign(+-0) = sign(NaN) = +0
"""
import numpy as np

import _sgd_oracle as SO
from oracle import choco_oracle as O

F32 = np.float32
ACCUM, APPLY, DIV, SCALE = 1, 2, 4, 8  # CHOCO_EF_*
MODES = [ACCUM, APPLY, APPLY | DIV, APPLY | SCALE, APPLY | DIV | SCALE]


def add32(a, b):
    with np.errstate(all="ignore"):
        return (np.asarray(a, F32) + np.asarray(b, F32)).astype(F32)


def sub32(a, b):
    with np.errstate(all="ignore"):
        return (np.asarray(a, F32) - np.asarray(b, F32)).astype(F32)


def div32(a, b):
    with np.errstate(all="ignore"):
        return (np.asarray(a, F32) / np.asarray(b, F32)).astype(F32)


def accum(flat, x):
    """flat after ACCUM; x the params widened to fp32."""
    return add32(flat, x)


def apply(flat, x, divisor=None, lr=None, dtype="fp32"):
    """(params_new on the dtype's grid, flat after) of APPLY with DIV (divisor given) and SCALE
    (lr given)."""
    a = np.asarray(flat, F32)
    if divisor is not None:
        a = div32(a, F32(divisor))
    flat_out = a
    if lr is not None:
        a = SO.mul32(F32(-lr), a)
    return SO.to_grid(add32(x, a), dtype), flat_out


def ef(mode, flat, x, lr, divisor, dtype="fp32"):
    """(params_new, flat after) of one choco_params_ef call."""
    if mode & ACCUM:
        return SO.to_grid(x, dtype), accum(flat, x)
    return apply(flat, x, divisor if mode & DIV else None, lr if mode & SCALE else None, dtype)


def residual(x, norms, lens):
    """(resid, u) of choco_sign_local_residual."""
    u = O.sign_local(x, norms, lens)
    return sub32(x, u), u
