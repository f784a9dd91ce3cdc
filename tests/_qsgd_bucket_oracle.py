"""numpy fp32 restatement of the bucketed QSGD contract (include/choco_codec.h "bucketed QSGD"):
every operation one fp32 rounding, in the header's order."""
import numpy as np

from oracle import choco_oracle as O

F32 = np.float32


def align16(b):
    return (b + 15) // 16 * 16


def biased_c(q, B, is_biased):
    s = float(2 ** q - 1)
    return F32(1.0 / (min(B / s ** 2, np.sqrt(float(B)) / s) + 1.0)) if is_biased else F32(1.0)


def bucket_max(d, B):
    """m_b: max |d| over the bucket's non-NaN elements (0 if none); the last bucket may be short."""
    nb = -(-d.size // B)
    a = np.full(nb * B, np.nan, dtype=F32)
    a[:d.size] = np.abs(d)
    return np.fmax.reduce(a.reshape(nb, B), axis=1, initial=F32(0)).astype(F32)


def decode(m, level, neg, q, B, is_biased=False):
    with np.errstate(invalid="ignore", over="ignore"):
        cm = (biased_c(q, B, is_biased) * m).astype(F32)
        t = ((np.repeat(cm, B)[:level.size] * level.astype(F32)).astype(F32) / F32(2 ** q - 1)).astype(F32)
    return np.where(neg, -t, t).astype(F32)


def quantize(d, q, B, u, is_biased=False):
    """(scales, levels, sign bits, dense decode, message bytes) of the delta d with uniforms u."""
    d = np.asarray(d, dtype=F32)
    s = F32(2 ** q - 1)
    m = bucket_max(d, B)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        lf = ((s * np.abs(d)).astype(F32) / np.repeat(m, B)[:d.size]).astype(F32)
        pl = np.floor(lf).astype(F32)
        lvl = (pl + (np.asarray(u, dtype=F32) < (lf - pl).astype(F32)).astype(F32)).astype(F32)
    level = np.where(np.isnan(lvl), 0, np.minimum(lvl, s)).astype(np.int64)
    neg = d < 0
    head = np.zeros(align16(4 * m.size) // 4, dtype=F32)
    head[:m.size] = m
    msg = np.concatenate([head.view(np.uint8), O.qsgd_pack(level.astype(F32), d, q)])
    return m, level, neg, decode(m, level, neg, q, B, is_biased), msg


def split(msg, n, q, B):
    """(scales, levels, sign bits) read back from message bytes."""
    nb = -(-n // B)
    sb = align16(4 * nb)
    level, neg = O.qsgd_unpack(np.asarray(msg[sb:]), n, q)
    return np.asarray(msg[:sb]).view(F32)[:nb].copy(), level.astype(np.int64), neg
