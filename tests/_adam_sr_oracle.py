"""numpy restatement of choco_params_adam_sr (include/choco_codec.h, "choco_params_adam_sr" and
the lanes of "stochastic rounding for bf16 models"), written from the header and not from the
kernel.  For a bf16 tensor, element with flat index i:

    p, g, m, v widened to fp32 (first: m = v = +0)
    the lines of _adam_oracle.adam_step(dtype="fp32", narrow_coef=False): every line fp32, nothing
    narrowed between the lines, the clip product c * g not narrowed, den and q from the unrounded
    v_new and m_new
    exp_avg = sr(m_new, lane 1);  exp_avg_sq = sr(v_new, lane 2);  param = sr(p_new, lane 0)
    flat = p_new, unrounded;  the clipped gradient, where stored, is c * g rounded to nearest

with sr(x, lane) = the rounding below with the 16 bits of (seed, step, lane, i):

    mix(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
             return z ^ (z >> 31)
    key_0 = mix(seed + (step + 1) * 0xD1B54A32D192ED03);  key_L = mix(key_0 + L * 0xD1B54A32D192ED03)
    w = mix(key_L + ((i >> 2) + 1) * 0x9E3779B97F4A7C15);  r16 = (w >> (16 * (i & 3))) & 0xffff
    u = bits(x):  inf kept, NaN -> 0x7fc0, otherwise (u + r16) >> 16

An fp32 tensor of the same model takes _adam_oracle.adam_step(dtype="fp32") and draws no bits.
The integer arithmetic is Python's own, reduced modulo 2^64 by hand: a second implementation
beside chocosgd_amd/rounding.py's numpy one.
"""
import numpy as np

import _adam_oracle as AO
from _sgd_oracle import F32, to_grid

M64 = (1 << 64) - 1
STEP_GAMMA = 0xD1B54A32D192ED03
GOLDEN_GAMMA = 0x9E3779B97F4A7C15


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def lane_key(seed, step, lane):
    key = mix((seed + (step + 1) * STEP_GAMMA) & M64)
    return key if lane == 0 else mix((key + lane * STEP_GAMMA) & M64)


def bits16(seed, step, start, n, lane):
    """r16 of flat elements start .. start + n - 1 in lane `lane`, a uint32 array."""
    key = lane_key(seed, step, lane)
    if n == 0:
        return np.empty(0, dtype=np.uint32)
    q0, q1 = start >> 2, (start + n - 1) >> 2
    words = np.array([mix((key + (q + 1) * GOLDEN_GAMMA) & M64) for q in range(q0, q1 + 1)], dtype=np.uint64)
    i = np.arange(start, start + n, dtype=np.uint64)
    w = words[((i >> np.uint64(2)) - np.uint64(q0)).astype(np.int64)]
    return ((w >> (np.uint64(16) * (i & np.uint64(3)))) & np.uint64(0xFFFF)).astype(np.uint32)


def sr_narrow(x, r16):
    """The stochastic rounding of the fp32 array x with the bits r16: fp32 values on the bf16 grid."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    mag = u & 0x7FFFFFFF
    out = ((u + r16.astype(np.uint64)) >> 16) & 0xFFFF
    out = np.where(mag == 0x7F800000, u >> 16, out)
    out = np.where(mag > 0x7F800000, 0x7FC0, out)
    return (out.astype(np.uint32) << 16).view(F32)


def adam_sr_step(p, g, m, v, lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, step=1, decoupled=False, first=False,
                 coef=None, dtype="bf16", seed=0, sr_step=0, start=0):
    """One update of a tensor whose first element has flat index `start`.  p, g, m, v: fp32
    arrays on the dtype's grid.  Returns (param as stored, exp_avg, exp_avg_sq, the clipped
    gradient as WRITE_CLIPPED stores it, flat): fp32 arrays, the first four on the dtype's grid."""
    if dtype == "fp32":
        p_new, m_new, v_new, gc = AO.adam_step(p, g, m, v, lr, beta1, beta2, eps, wd, step, decoupled, first, coef,
                                               dtype="fp32")
        return p_new, m_new, v_new, gc, p_new
    assert dtype == "bf16", "fp16 has no stochastic rounding"
    p_new, m_new, v_new, gc = AO.adam_step(p, g, m, v, lr, beta1, beta2, eps, wd, step, decoupled, first, coef,
                                           dtype="fp32", narrow_coef=False)
    n = p_new.size
    lanes = [bits16(seed, sr_step, start, n, lane) for lane in range(3)]
    return (sr_narrow(p_new, lanes[0]), sr_narrow(m_new, lanes[1]), sr_narrow(v_new, lanes[2]), to_grid(gc, "bf16"),
            p_new)
