"""numpy restatement of the MX wire's contract (include/choco_codec.h "MX wire"): power-of-two block
scales from the bits of the block maximum, E2M1 / E4M3 codes rounded to nearest even or by the
hardware's stochastic rule from the restated random stream.  Grid arithmetic is exact in float64."""
import numpy as np

from oracle import choco_oracle as O

F32 = np.float32
BLOCK = 32
U64 = np.uint64
# code magnitude -> value; E4M3 (OCP): bias 7, subnormals m 2^-9, 0x7F is NaN and never sent
GRID = {4: np.array([0, .5, 1, 1.5, 2, 3, 4, 6]),
        8: np.array([(c & 7) * 2.0 ** -9 if c < 8 else (1 + (c & 7) / 8) * 2.0 ** ((c >> 3) - 7) for c in range(127)])}
BIAS, THR, SIGN = {4: 2, 8: 8}, {4: 0x400000, 8: 0x600000}, {4: 8, 8: 128}


def align16(b):
    return (b + 15) // 16 * 16


def packed_bytes(n, q):
    return align16(-(-n // BLOCK)) + align16((n * q + 7) // 8)


def scale_bytes(d, q):
    """One byte per block: e + 127 from the bits of amax alone, 0 for a zero block, 0xFF for inf / NaN."""
    nb = -(-d.size // BLOCK)
    k = np.zeros(nb * BLOCK, dtype=np.uint32)
    k[:d.size] = np.asarray(d, dtype=F32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    k = k.reshape(nb, BLOCK).max(axis=1).astype(np.int64)
    t = (k >> 23) - BIAS[q] + ((k & 0x7FFFFF) > THR[q])
    return np.where(k >= 0x7F800000, 255, np.maximum(t, 0)).astype(np.uint8)


def brackets(d, sb, q):
    """(|d| / 2^e, lower grid index, upper grid index) per element, in float64 (exact)."""
    G = GRID[q]
    e = np.repeat(sb.astype(np.int64) - 127, BLOCK)[:d.size]
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.nan_to_num(np.abs(d.astype(np.float64)) * 2.0 ** -e.astype(np.float64), nan=0.0, posinf=0.0)
    lo = np.clip(np.searchsorted(G, a, "right") - 1, 0, len(G) - 1)
    return a, lo, np.minimum(lo + 1, len(G) - 1)


def random_words(n, seed, offset, q):
    """The 32-bit random operand of every element's conversion: stream and position as
    O.qsgd_uniforms_at; conversion c of a stream (E4M3: the element's position, E2M1: its pair's)
    takes the high (c even) or low half of xoroshiro output c >> 1; the second element of an E2M1
    pair takes its pair's operand rotated left by one."""
    e = np.arange(n, dtype=U64)
    key = U64(O.qrng_key(seed, offset))
    o = e & U64(8191)
    g = o >> U64(11)
    sid = ((e >> U64(13)) << U64(9)) | ((g >> U64(1)) << U64(8)) | ((o >> U64(3)) & U64(255))
    pos = (g & U64(1)) * U64(8) + (e & U64(7))
    c = pos >> U64(1) if q == 4 else pos
    j = c >> U64(1)
    with np.errstate(over="ignore"):
        z = key + (U64(2) * sid + U64(1)) * U64(O.GAMMA)
        s0, s1 = O.splitmix64_mix(z), O.splitmix64_mix(z + U64(O.GAMMA))
        out = np.zeros(n, dtype=U64)
        for step in range(8):
            out[j == U64(step)] = (s0 + s1)[j == U64(step)]
            t = s1 ^ s0
            s0, s1 = O._rotl64(s0, 24) ^ t ^ (t << U64(16)), O._rotl64(t, 37)
    r = np.where((c & U64(1)) == 0, out >> U64(32), out & U64(0xFFFFFFFF))
    if q == 4:
        r = np.where((e & U64(1)) == 1, ((r << U64(1)) | (r >> U64(31))) & U64(0xFFFFFFFF), r)
    return r


def decode(sb, codes, q):
    """grid[code] 2^e with the code's sign; NaN throughout a 0xFF block."""
    e = np.repeat(sb.astype(np.int64) - 127, BLOCK)[:codes.size].astype(np.float64)
    mag = GRID[q][codes & (SIGN[q] - 1)] * 2.0 ** e
    v = np.where(codes & SIGN[q], -mag, mag).astype(F32)
    v[np.repeat(sb == 255, BLOCK)[:codes.size]] = np.nan
    return v


def pack(sb, codes, n, q):
    head = np.zeros(align16(sb.size), dtype=np.uint8)
    head[:sb.size] = sb
    body = np.zeros(align16((n * q + 7) // 8), dtype=np.uint8)
    if q == 8:
        body[:n] = codes
    else:
        c = np.zeros(2 * ((n + 1) // 2), dtype=np.uint8)
        c[:n] = codes
        body[:c.size // 2] = c[0::2] | (c[1::2] << 4)
    return np.concatenate([head, body])


def split(msg, n, q):
    """(scale bytes, one code per element) read back from message bytes."""
    nb = -(-n // BLOCK)
    body = np.asarray(msg[align16(nb):])
    codes = body[:n] if q == 8 else np.stack([body & 15, body >> 4], axis=1).reshape(-1)[:n]
    return np.asarray(msg[:nb]).copy(), codes.astype(np.uint8)


def quantize(d, q, sr=False, seed=0, offset=0):
    """(scale bytes, codes, dense decode, message bytes) of the delta d."""
    d = np.asarray(d, dtype=F32)
    sb = scale_bytes(d, q)
    G = GRID[q]
    a, lo, hi = brackets(d, sb, q)
    gap = np.where(hi > lo, G[hi] - G[lo], 1.0)
    if sr:  # up iff floor(f 2^32) + r >= 2^32
        f32 = np.floor((a - G[lo]) / gap * 2.0 ** 32)
        up = f32 + random_words(d.size, seed, offset, q).astype(np.float64) >= 2.0 ** 32
    else:  # nearest, ties to the even code
        dl, dh = a - G[lo], G[hi] - a
        up = (dh < dl) | ((dh == dl) & (hi % 2 == 0))
    codes = (np.where(up, hi, lo) | np.where(np.signbit(d), SIGN[q], 0)).astype(np.uint8)
    codes[np.repeat((sb == 0) | (sb == 255), BLOCK)[:d.size]] = 0
    return sb, codes, decode(sb, codes, q), pack(sb, codes, d.size, q)
