"""numpy restatement of the per-element update of choco_params_sgd (include/choco_codec.h;
apply_gradient, dl_code/pcode/optim/utils.py:13-47).  Each line is one reference op with one
rounding:

    d = g
    if wd  != 0:  d   = fma(wd, p, d)
    if mom != 0:  t   = buf * mom
                  buf = first ? fma(1, d, 0 * mom) : fma(1 - damp, d, t)
                  d   = nesterov ? fma(mom, buf, d) : buf
    p_new = fma(-lr, d, p)

dtype "fp32": plain fp32.  "bf16" / "fp16" (the `scalars_fp32` model): operands and results
are fp32 arrays holding values of the 16-bit grid; every line is computed in fp32 and narrowed
round-to-nearest-even to the grid after that line, the scalars stay fp32.
"""
import numpy as np

F32 = np.float32


def fma32(a, b, c):
    """fmaf(a, b, c) with ONE rounding, elementwise on fp32 inputs, on any interpreter (no
    math.fma needed).  The float64 product of two fp32 values is exact; the float64 sum is
    corrected to round-to-odd with a TwoSum, so that the final narrowing to fp32 rounds the
    exact a * b + c (no double rounding)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(all="ignore"):
        x = a.astype(np.float64) * b.astype(np.float64)  # exact: 24 x 24 bits
        y = c.astype(np.float64)
        s = np.ascontiguousarray(x + y)
        bb = s - x
        err = (x - (s - bb)) + (y - bb)                  # exactly x + y - s for finite s
        # round to odd: of the two doubles around the exact sum, the one with an odd mantissa
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def mul32(a, b):
    with np.errstate(all="ignore"):
        return (np.asarray(a, F32) * np.asarray(b, F32)).astype(F32)


def to_grid(v, dtype):
    """v (fp32) narrowed round-to-nearest-even to `dtype` and widened again."""
    v = np.ascontiguousarray(v, dtype=F32)
    if dtype == "fp32":
        return v
    if dtype == "fp16":
        with np.errstate(all="ignore"):
            return v.astype(np.float16).astype(F32)
    assert dtype == "bf16", dtype
    u = v.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    out = (r & 0xFFFFFFFF).astype(np.uint32).view(F32)
    return np.where(np.isnan(v), F32(np.nan), out).astype(F32)


def scalars(lr, wd, mom, damp):
    """torch's conversion of a Python scalar for an fp32 tensor."""
    return F32(-lr), F32(wd), F32(mom), F32(1.0 - damp)


def sgd_step(p, g, buf, lr, wd=0.0, mom=0.0, damp=0.0, nesterov=False, first=False, dtype="fp32"):
    """One update.  Returns (p_new, buf_new or None, d_p) as fp32 arrays (on the dtype's grid)."""
    nlr, wdf, momf, omd = scalars(lr, wd, mom, damp)
    p, d = np.asarray(p, F32), np.asarray(g, F32)
    if wd != 0:
        d = to_grid(fma32(wdf, p, d), dtype)
    buf_new = None
    if mom != 0:
        if first:
            buf_new = to_grid(fma32(F32(1), d, mul32(F32(0), momf)), dtype)
        else:
            t = to_grid(mul32(buf, momf), dtype)
            buf_new = to_grid(fma32(omd, d, t), dtype)
        d = to_grid(fma32(momf, buf_new, d), dtype) if nesterov else buf_new
    return to_grid(fma32(nlr, d, p), dtype), buf_new, d
