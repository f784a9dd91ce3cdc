"""The numpy model of choco_params_consensus (include/choco_codec.h, consensus evaluation).  Per
flat index i, element j of tensor s, every line with one rounding:

    a = fdiv(xsum[i], divisor)                   _allreduce_oracle.fdiv: a correctly rounded division
    x = master[i] if master is given else params[s][j] widened
    d = a - x                                    fp32
    DIST:       ssd_s += (double)d * d,  ssa_s += (double)a * a
    WRITE_AVG:  avg_out[s][j] = to_grid(a, dtype_s)     _sgd_oracle.to_grid

and the sums in the kernels' fixed order: one partial per (8192-element tile, tensor) pair -- a
span of at most 1024 elements by one wave (lane l adds elements l, l + 64, ... of the span; the xor
butterfly 32 .. 1 joins the lanes), a longer one by 256 threads (the 8-element group at absolute
flat offset 8 g belongs to thread (g - first group of the span) mod 256; groups and their elements
in ascending order; the butterfly per wave, then ((w0 + w1) + w2) + w3) -- a tensor's partials in
ascending tile order, the tensors in ascending order.

    out = [float32(sqrt(sum_s ssd_s)), float32(sqrt(sum_s ssa_s))],  dists[s] = float32(sqrt(ssd_s))
"""
import numpy as np

from _allreduce_oracle import fdiv
from _sgd_oracle import F32, to_grid

TILE, WAVE_MAX = 8192, 1024
_LANES = np.arange(64)


def _butterfly(acc):
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., _LANES ^ o]
    return acc[..., 0]


def span_sum(sq, a):
    """sq: the fp64 squares of flat elements [a, a + len(sq)) of one tensor inside one tile."""
    m = sq.size
    if m <= WAVE_MAX:
        rows = np.concatenate([sq, np.zeros(-m % 64)]).reshape(-1, 64)
        acc = np.zeros(64)
        for r in rows:
            acc = acc + r
        return _butterfly(acc)
    lead = a & 7
    cells = np.concatenate([np.zeros(lead), sq, np.zeros(-(lead + m) % 2048)]).reshape(-1, 256, 8)
    acc = np.zeros(256)
    for it in range(cells.shape[0]):
        for k in range(8):
            acc = acc + cells[it, :, k]
    w = _butterfly(acc.reshape(4, 64))
    return ((w[0] + w[1]) + w[2]) + w[3]


def ordered_sums(values, lens):
    """Per tensor, the fp64 sum of squares of the flat fp32 `values` in the kernels' order."""
    with np.errstate(all="ignore"):
        sq = np.asarray(values, F32).astype(np.float64) ** 2
        out, o0 = [], 0
        for m in lens:
            acc, a = np.float64(0), o0
            while a < o0 + m:
                b = min(o0 + m, (a // TILE + 1) * TILE)
                acc = acc + span_sum(sq[a:b], a)
                a = b
            out.append(acc)
            o0 += m
        return np.array(out, dtype=np.float64)


def total(sums):
    acc = np.float64(0)
    with np.errstate(all="ignore"):
        for s in sums:
            acc = acc + s
    return acc


def consensus(x, xsum, divisor, lens, dtypes):
    """x: the flat fp32 view of this worker's parameters (values of each tensor's grid) or its
    master copy; xsum: the flat all-reduced sum.  dtypes: one of "fp32" / "bf16" / "fp16" per
    tensor.  Returns (avg, out, dists): avg the flat fp32 array of what WRITE_AVG leaves (each
    tensor on its dtype's grid), out the two fp32 stats, dists the per-tensor distances."""
    a = fdiv(xsum, divisor)
    with np.errstate(all="ignore"):
        d = (a - np.asarray(x, F32)).astype(F32)
        ssd, ssa = ordered_sums(d, lens), ordered_sums(a, lens)
        out = np.sqrt(np.array([total(ssd), total(ssa)])).astype(F32)
        dists = np.sqrt(ssd).astype(F32)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    avg = np.concatenate([to_grid(a[offs[s]:offs[s + 1]], dtypes[s]) for s in range(len(lens))] + [np.zeros(0, F32)])
    return avg.astype(F32), out, dists


def adjacent(a, b):
    """Equal or neighbouring fp32 values (finite, same sign)."""
    return abs(int(F32(a).view(np.uint32)) - int(F32(b).view(np.uint32))) <= 1


def ulp32(v):
    return float(np.spacing(F32(v)))
