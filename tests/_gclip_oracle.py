"""numpy restatement of global-norm gradient clipping as choco_params_gradnorm and
choco_params_sgd_gclip compute it (include/choco_codec.h; torch.nn.utils.clip_grad_norm_,
dl_code/pcode/distributed_running_nlp.py:96), on top of _sgd_oracle.  With CD the coefficient's
dtype ("fp32" / "bf16" / "fp16"), every line one torch op with one rounding:

    total = rnd_CD((float)sqrt(fp64 sum of g^2 over every tensor))
    t = rnd_CD(total + (float)1e-6);  r = rnd_CD(1.0f / t);  c = rnd_CD(r * (float)max_norm)
    c = c > 1 ? 1 : c                                     a NaN stays NaN
    g = rnd_DT(c * g)
"""
import numpy as np

from _sgd_oracle import F32, mul32, to_grid


def common_dtype(dtypes):
    """All bf16 -> bf16, all fp16 -> fp16, any fp32 or any mix -> fp32."""
    kinds = set(dtypes)
    return kinds.pop() if len(kinds) == 1 else "fp32"


def total64(grads):
    """sqrt of the fp64 sum of squares over every element of every array (None: no gradient)."""
    acc = np.float64(0)
    with np.errstate(all="ignore"):
        for g in grads:
            if g is not None:
                v = np.asarray(g, F32).astype(np.float64)
                acc = acc + np.sum(v * v)
        return np.sqrt(acc)


def total(grads, cd="fp32"):
    with np.errstate(all="ignore"):
        return to_grid(np.array([total64(grads)]).astype(F32), cd)[0]


def coef(total_norm, max_norm, cd="fp32"):
    """The clip coefficient from a total on CD's grid."""
    one = lambda v: to_grid(np.array([v], F32), cd)[0]  # noqa: E731
    with np.errstate(all="ignore"):
        t = one(F32(one(total_norm)) + F32(1e-6))
        r = one(F32(1.0) / t)
        c = one(mul32(r, F32(max_norm)))
    return F32(1.0) if c > 1 else F32(c)


def clip(g, c, dtype="fp32"):
    """rnd_DT(c * g): c in fp32 times the widened g, narrowed once."""
    return to_grid(mul32(F32(c), np.asarray(g, F32)), dtype)


def ulp_distance(a, b, cd="fp32"):
    """|a - b| in units of CD's grid spacing (finite positive values)."""
    shift = {"fp32": 0, "bf16": 16, "fp16": None}[cd]
    if shift is None:
        return abs(int(np.float16(a).view(np.uint16)) - int(np.float16(b).view(np.uint16)))
    return abs((int(F32(a).view(np.uint32)) >> shift) - (int(F32(b).view(np.uint32)) >> shift))
