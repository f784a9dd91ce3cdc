"""Input builders for the sender-kernel edge tests (plain numpy, no GPU).

The QSGD quantize divides s * |d| by the norm with a fast form that is claimed correctly
rounded only for norm in [2^-30, 2^96] and a first quotient q0 in [2^-60, 2^7]; everything
else must reach the IEEE division (csrc/qsgd.hip QDiv, DESIGN.md section 4 "Division").  The
guard is taken per 8-element group and a flagged group sends its whole wave through the
slow branch, so the inputs here put values a few ulps on both sides of every threshold, at
chosen places of the 8192-element tiles:

  SN = 3 * 8192 + 37: three full tiles (the fast path) and a partial tile (the out-of-line
  slow tile: four full groups and a 5-element group).
  "ragged": boundaries group-aligned inside tile 0 (5000), mid-group (8195), one past a tile
  edge (16385) and on a tile edge (24576): every full tile crosses a tensor boundary.

A 512-element aligned slab of a full tile is what one wave handles at one group step, in
both kernel shapes (256 threads x 4 groups, 512 threads x 2 groups).  `pinned_delta` makes
slabs with no flagged group, with only flagged groups and with both.

`classify` restates the guard from the documented ranges, not from the kernel's code.
tests/test_sender_edges_host.py holds the builders to the coverage the GPU tests rely on.
"""
import functools

import numpy as np

F32 = np.float32
U32 = np.uint32

SN = 3 * 8192 + 37
TILE = 8192
SLAB = 512
QLAYOUTS = {"flat": [SN], "ragged": [5000, 3195, 8190, 8191, 37]}
assert sum(QLAYOUTS["ragged"]) == SN

T_LO_FACTOR = F32(float.fromhex("0x1.00001p-60"))
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45,
                     np.finfo(F32).tiny, np.finfo(F32).max], dtype=F32)


def frozen(a):
    a.flags.writeable = False
    return a


def bounds(lens):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return list(zip(off[:-1].tolist(), off[1:].tolist()))


def f32(x):
    return np.asarray(x, dtype=F32)


def step_ulps(v, k):
    """The fp32 value k steps from the positive finite v (towards +inf for k > 0)."""
    b = int(f32(v).view(U32)) + int(k)
    return np.array([max(0, min(b, 0x7F800000))], dtype=U32).view(F32)[0]


def prev32(v):
    return step_ulps(v, -1)


def next32(v):
    return step_ulps(v, 1)


def ordered(a):
    """fp32 -> int64 in value order (adjacent floats differ by one; +0 and -0 coincide)."""
    b = f32(a).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def within_one_ulp(got, want):
    """Per element: the same value, the adjacent fp32 value, or the same class for 0, inf and
    NaN (the bound of the device norms: both sides sum exact fp64 terms, rounded once)."""
    got, want = f32(got), f32(want)
    special = ~np.isfinite(got) | ~np.isfinite(want) | (got == 0) | (want == 0)
    same_class = (np.isnan(got) & np.isnan(want)) | (got == want)
    near = np.abs(ordered(got) - ordered(want)) <= 1
    return np.where(special, same_class, near)


def base_norm(N):
    """The norm the edge magnitudes are built around: N itself, or 1.0 where N is 0, inf or
    NaN (a ladder around those would hold nothing but 0, inf and NaN)."""
    N = F32(N)
    return N if np.isfinite(N) and N > 0 else F32(1.0)


# ------------------------------------------------------------------------------ QSGD ladder
@functools.lru_cache(maxsize=None)
def _ladder(Nbits, s):
    N = np.array([Nbits], dtype=U32).view(F32)[0]
    sf = F32(s)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        geo = [((N * F32(2.0 ** e)) * F32(1 + j / 8)) / sf for e in range(-70, 13) for j in range(8)]
        lo_c = (N * T_LO_FACTOR) / sf
        hi_c = (F32(128.0) * N) / sf
    lo = [step_ulps(lo_c, k) for k in range(-3, 4)] if np.isfinite(lo_c) and lo_c > 0 else [lo_c] * 7
    hi = [step_ulps(hi_c, k) for k in range(-3, 4)] if np.isfinite(hi_c) and hi_c > 0 else [hi_c] * 7
    top = [step_ulps(N, k) for k in range(-2, 3)]
    return frozen(np.array(geo + lo + hi + top + SPECIALS.tolist(), dtype=F32))


def ladder(N, s):
    """The edge magnitudes for the norm N and s = 2^q - 1 levels, all computed in fp32:
    N 2^e (1 + j/8) / s for e = -70..12, j = 0..7; -3..+3 ulps around N 0x1.00001p-60 / s (the
    low threshold on t = s |d|) and around 128 N / s (q0 = 128); -2..+2 ulps around N (the top
    level s exactly, and the container clamp one step above); +-0, +-inf, NaN, +-1e-45,
    FLT_MIN, FLT_MAX."""
    return _ladder(int(base_norm(N).view(U32)), int(s))


N_TAIL_LADDER = SN - 3 * TILE  # the partial tile takes the ladder's last 37 entries


def classify(d, N, s):
    """(low, high) per element, from the documented ranges: with t = RN(s |d|),
    low = t != 0 and t < RN(N 0x1.00001p-60); high = not (RN(t RN(1/N)) <= 128) (so inf and
    NaN are high).  A group holding a low or high element must take the IEEE division."""
    N = F32(N)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        t = (F32(s) * np.abs(f32(d))).astype(F32)
        low = (t != 0) & (t < N * T_LO_FACTOR)
        q0 = (t * (F32(1.0) / N)).astype(F32)
        high = ~(q0 <= F32(128.0))
    return low, high


def group_flags(d, N, s):
    """Per 8-element group of d (len a multiple of 8): holds a low or high element."""
    low, high = classify(d, N, s)
    return (low | high).reshape(-1, 8).any(axis=1)


def slab_classes(d, N, s, ntile=3):
    """(mixed, none, all): 512-element slabs of the first `ntile` full tiles that hold both
    flagged and unflagged groups, no flagged group, only flagged groups."""
    g = group_flags(d[:ntile * TILE], N, s).reshape(-1, SLAB // 8)
    cnt = g.sum(axis=1)
    return int(((cnt > 0) & (cnt < SLAB // 8)).sum()), int((cnt == 0).sum()), int((cnt == SLAB // 8).sum())


def _filler(rng, n, N, s):
    """d = +-N lf / s with lf ~ U(0, min(s, 100)): levels, not randn, so the fast division stays
    populated at every q (randn fillers at q >= 9 put s |d| / norm above 128 nearly everywhere)."""
    lf = rng.uniform(0.0, min(s, 100), size=n).astype(F32)
    sg = np.where(rng.random(n) < 0.5, F32(-1), F32(1))
    with np.errstate(over="ignore", under="ignore"):
        return (sg * ((base_norm(N) * lf) / F32(s))).astype(F32)


def _signed(rng, lad):
    """The ladder with random signs on all but its special values (which carry their own)."""
    out = lad.copy()
    m = lad.size - SPECIALS.size
    out[:m] = np.where(rng.random(m) < 0.5, -out[:m], out[:m])
    return out


def _sprinkle(rng, d, is_ladder, lo, hi, vals):
    """vals at distinct seeded positions of [lo, hi), in shuffled order."""
    pos = lo + rng.choice(hi - lo, size=min(vals.size, hi - lo), replace=False)
    d[pos] = rng.permutation(vals)[:pos.size]
    is_ladder[pos] = True


def _fill_segment(rng, d, is_ladder, a, b, N, s):
    """One tensor [a, b) of `ragged`, built around its own norm with the same ladder: filler,
    the ladder's tail (thresholds, top level, specials) at the tensor's two ends, and one
    shuffled ladder copy per 8192 elements in between."""
    d[a:b] = _filler(rng, b - a, N, s)
    lad = _signed(rng, ladder(N, s))
    edge = lad[-N_TAIL_LADDER:]
    k = min(edge.size, b - a)
    d[a:a + k] = rng.permutation(edge)[:k]
    is_ladder[a:a + k] = True
    if b - a > 4 * k:
        d[b - k:b] = rng.permutation(edge)[:k]
        is_ladder[b - k:b] = True
        for c in range(max(1, (b - a) // TILE)):
            _sprinkle(rng, d, is_ladder, a + k, b - k, lad)


@functools.lru_cache(maxsize=None)
def _pinned_delta(Nbits, s, seed):
    N = np.array([Nbits], dtype=U32).view(F32)[0]
    rng = np.random.default_rng([seed, s, Nbits])
    d = _filler(rng, SN, N, s)
    is_ladder = np.zeros(SN, dtype=bool)
    lad = ladder(N, s)
    _sprinkle(rng, d, is_ladder, 0, TILE, _signed(rng, lad))               # tile 0
    _sprinkle(rng, d, is_ladder, 2 * TILE, 3 * TILE, _signed(rng, lad))    # tile 2
    d[3 * TILE:] = rng.permutation(_signed(rng, lad)[-N_TAIL_LADDER:])     # the partial tile
    is_ladder[3 * TILE:] = True
    # tile 1: one flagged ladder value in every group of its first half, filler in its second
    low, high = classify(lad, base_norm(N), s)
    flagged = lad[low | high] if (low | high).any() else lad
    g0 = TILE + 8 * np.arange(TILE // 16)
    pos = g0 + rng.integers(0, 8, size=g0.size)
    d[pos] = flagged[rng.integers(0, flagged.size, size=g0.size)]
    is_ladder[pos] = True
    return frozen(d), frozen(is_ladder)


def pinned_delta(N, s, seed=0):
    """(d, is_ladder) on `flat` for the pinned norm N: a level-driven filler; shuffled copies
    of the ladder at seeded positions of tile 0 and tile 2 and the ladder's last 37 entries
    (thresholds, top level, specials) in the partial tile; in the first 4096 elements of tile 1
    one flagged ladder value per 8-group, in its last 4096 filler only."""
    return _pinned_delta(int(F32(N).view(U32)), int(s), int(seed))


@functools.lru_cache(maxsize=None)
def _ragged_delta(norm_bits, s, seed):
    norms = np.array(norm_bits, dtype=U32).view(F32)
    rng = np.random.default_rng([seed, s, 77])
    d = np.zeros(SN, dtype=F32)
    is_ladder = np.zeros(SN, dtype=bool)
    for (a, b), N in zip(bounds(QLAYOUTS["ragged"]), norms):
        _fill_segment(rng, d, is_ladder, a, b, N, s)
    return frozen(d), frozen(is_ladder)


def ragged_delta(norms, s, seed=0):
    """(d, is_ladder) on `ragged`: every tensor built around its own pinned norm."""
    return _ragged_delta(tuple(int(b) for b in f32(norms).view(U32)), int(s), int(seed))


def under_xhat(d, is_ladder, seed=0):
    """(x, xhat) whose delta is d: at ladder positions xhat = d, x = 2 d where 2 d is finite
    and d != 0, otherwise xhat = +0, x = d -- there x - xhat == d exactly (bit for bit, -0
    included).  Elsewhere xhat = d r for a random |r| in [0.5, 3) and x = fl(d + xhat), so
    fl(x - xhat) is d to within a few ulps of x.  The reference of a test is fl(x - xhat)."""
    rng = np.random.default_rng([seed, 4242])
    d = f32(d)
    r = (rng.uniform(0.5, 3.0, size=d.size) * np.where(rng.random(d.size) < 0.5, -1, 1)).astype(F32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        xhat = (d * r).astype(F32)
        x = (d + xhat).astype(F32)
        d2 = (d + d).astype(F32)
    dbl = is_ladder & np.isfinite(d2) & (d != 0)
    one = is_ladder & ~dbl
    xhat[dbl], x[dbl] = d[dbl], d2[dbl]
    xhat[one], x[one] = F32(0), d[one]
    return x, xhat


def delta_of(x, xhat):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return (f32(x) - f32(xhat)).astype(F32) if xhat is not None else f32(x)


def sharp_uniforms(d, lens, norms, s, seed):
    """Pinned uniforms that make the level depend on the last bit of s |d| / norm.  The
    quantize rounds up where u < lf - floor(lf), so the wire shows lf only through that one
    comparison; a quotient off by an ulp would pass under ordinary uniforms almost always.
    Here a third of the elements take u = lf - floor(lf) itself (the level stays at the floor),
    a third the fp32 value just below it (the level steps up) and a third an ordinary multiple
    of 2^-24, with lf the fp32 quotient of the delta d and its tensor's norm.  Elements whose
    fraction is 0 or NaN keep the ordinary value (or u = 0 for a fraction of 0)."""
    d = f32(d)
    u = uniforms(d.size, seed)
    kind = np.random.default_rng([seed, 31337]).integers(0, 3, size=d.size)
    with np.errstate(all="ignore"):
        nrm = np.concatenate([np.full(b - a, F32(norms[i])) for i, (a, b) in enumerate(bounds(lens))])
        lf = ((F32(s) * np.abs(d)).astype(F32) / nrm).astype(F32)
        frac = (lf - np.floor(lf)).astype(F32)
    ok = np.isfinite(frac) & (frac > 0)
    below = (frac.view(U32) - U32(1)).view(F32)
    u = np.where(ok & (kind == 0), frac, np.where(ok & (kind == 1), below, u)).astype(F32)
    u[np.isfinite(frac) & (frac == 0) & (kind == 0)] = F32(0)
    return u


def uniforms(n, seed):
    """Pinned uniforms in [0, 1) as torch.rand gives them (multiples of 2^-24), with 0 and
    the largest value below 1 among them."""
    rng = np.random.default_rng([seed, 99])
    u = (rng.integers(0, 1 << 24, size=n).astype(F32) * F32(2.0 ** -24)).astype(F32)
    u[rng.choice(n, size=64, replace=False)] = F32(0)
    u[rng.choice(n, size=64, replace=False)] = F32(1 - 2.0 ** -24)
    return u


# ------------------------------------------------------------------------------ sign pack
SIGN_N = 32 * 2049 + 5  # N' = 2050: two full 1024-word column blocks and a 2-word one
SIGN_LAYOUTS = {"flat": [SIGN_N], "ragged": [7, 33_000, 1, 31, 32_534]}
assert sum(SIGN_LAYOUTS["ragged"]) == SIGN_N
SIGN_ZERO_SEG, SIGN_NAN_SEG, SIGN_INF_SEG = 3, 1, 4   # of "ragged"
FINITE_KINDS = ("+0", "-0", "+sub", "-sub", "equal")
NONFINITE_KINDS = ("nan", "+inf", "-inf")


def sign_positions(n, lens):
    """Where the special values go: every tensor's first and last element, the buffer's first
    and last, both sides of every row boundary r N' of the (32, N') view, and the columns
    next to the last word's padding (the last real column and the first and last padded
    ones) in three rows."""
    Np = (n + 31) // 32
    pos = set()
    for a, b in bounds(lens):
        pos.update((a, b - 1))
    pos.update((0, n - 1))
    for r in range(1, 32):
        pos.update(p for p in (r * Np - 1, r * Np) if p < n)
    last_col = (n - 1) - 31 * Np
    for r in (0, 15, 30):
        pos.update(r * Np + c for c in (last_col, last_col + 1, Np - 1) if r * Np + c < n)
    return np.array(sorted(pos), dtype=np.int64)


def sign_specials(n, lens, seed=0, nonfinite=True):
    """(x_plain, x, xhat, mem, kinds): randn filler with NaN, +-inf, +-0, +-1e-45 and
    x == xhat (a delta of exactly +0) at sign_positions.  x_plain is the input of a call
    without xhat (the intended delta itself); (x, xhat) give that delta exactly at every
    special position (xhat = +0 there, or x == xhat != 0 for "equal") and fl(x - xhat) close
    to it elsewhere; mem == xhat at the special positions, so the fused consensus step adds
    +0 to x there.  With several tensors: tensor 3 is all zero (+0 and -0), NaN goes only
    into tensor 1 and inf only into tensor 4, so the other tensors' norms stay finite;
    nonfinite=False leaves NaN and inf out altogether (the ordinary case run after a
    non-finite one).  kinds: {position: kind}."""
    rng = np.random.default_rng([seed, n, len(lens)])
    segs = bounds(lens)
    d = rng.standard_normal(n).astype(F32)
    xhat = (rng.standard_normal(n) * 0.5).astype(F32)
    mem = rng.standard_normal(n).astype(F32)
    pos = sign_positions(n, lens)
    seg_of = np.searchsorted(np.array([b for _, b in segs]), pos, side="right")
    kinds = {}
    for i, (p, sg) in enumerate(zip(pos.tolist(), seg_of.tolist())):
        allowed = list(FINITE_KINDS)
        if nonfinite and (len(lens) == 1 or sg == SIGN_NAN_SEG):
            allowed.append("nan")
        if nonfinite and (len(lens) == 1 or sg == SIGN_INF_SEG):
            allowed += ["+inf", "-inf"]
        kinds[p] = allowed[(i + i // len(allowed)) % len(allowed)]
    if nonfinite and len(lens) > 1:  # at least one of each, wherever the cycle fell
        a, b = segs[SIGN_NAN_SEG]
        kinds[a + (b - a) // 2] = "nan"
        a, b = segs[SIGN_INF_SEG]
        kinds[a + (b - a) // 2], kinds[a + (b - a) // 3] = "+inf", "-inf"
    if len(lens) > 1:
        a, b = segs[SIGN_ZERO_SEG]
        for p in range(a, b):
            kinds[p] = "-0" if rng.random() < 0.5 else "+0"
    value = {"+0": 0.0, "-0": -0.0, "+sub": 1e-45, "-sub": -1e-45, "nan": np.nan, "+inf": np.inf, "-inf": -np.inf,
             "equal": 0.0}
    x = (d + xhat).astype(F32)
    for p, k in kinds.items():
        d[p] = F32(value[k])
        if k == "equal":
            x[p] = xhat[p]
        else:
            x[p], xhat[p] = d[p], F32(0)
        mem[p] = xhat[p]
    return d, x, xhat, mem, kinds
