"""numpy restatement of the dynamic loss scaling of choco_params_gradnorm_scaled and
choco_params_sgd[_master]_scaled (include/choco_codec.h), on top of _gclip_oracle and
_sgd_oracle.  The gradients are still multiplied by the loss scale; with CD the coefficient's
dtype, every line one rounding:

    inv   = (float)(1.0 / (double)scale)
    S     = fp64 sum of g^2 over every tensor;   found = !isfinite(S)
    total = rnd_CD((float)sqrt(S) * inv)
    c     = _gclip_oracle.coef(total, max_norm, CD), or 1 without a clip
    gc    = c * inv                                    fp32, not narrowed
    g     = rnd_DT(gc * g)       (master: gc * g in fp32, narrowed only where it is stored)
    out   = [total, gc, found, scale]

and torch's _amp_update_scale_ on (scale, tracker).
"""
import numpy as np

import _gclip_oracle as GO
from _sgd_oracle import F32, mul32, to_grid


def inv(scale):
    with np.errstate(all="ignore"):
        return F32(np.float64(1.0) / np.float64(F32(scale)))


def found(grads):
    """Whether the fp64 sum of squares is non-finite: exactly when some element is."""
    return not np.isfinite(GO.total64(grads))  # the root of the sum is finite exactly when the sum is


def total(grads, scale, cd="fp32"):
    """The norm of the unscaled gradient on CD's grid, from the fp64 root."""
    with np.errstate(all="ignore"):
        root = np.array([GO.total64(grads)]).astype(F32)
        return to_grid(mul32(root, inv(scale)), cd)[0]


def out(total_norm, max_norm, scale, is_found, cd="fp32"):
    """[total, gc, found, scale] from a total on CD's grid (max_norm None: no clip)."""
    c = F32(1.0) if max_norm is None else GO.coef(total_norm, max_norm, cd)
    return np.array([total_norm, mul32(c, inv(scale)), 1.0 if is_found else 0.0, scale], dtype=F32)


def unscale(g, gc, dtype="fp32"):
    """rnd_DT(gc * g); dtype "fp32" is also the master path's un-narrowed product."""
    return GO.clip(g, gc, dtype)


def update(scale, tracker, is_found, growth=2.0, backoff=0.5, interval=2000):
    """_amp_update_scale_: returns the new (scale, tracker)."""
    scale = F32(scale)
    with np.errstate(all="ignore"):
        if is_found:
            return F32(np.float64(scale) * np.float64(backoff)), 0
        if tracker + 1 == interval:
            s = F32(np.float64(scale) * np.float64(growth))
            return (s if np.isfinite(s) else scale), 0
    return scale, tracker + 1
