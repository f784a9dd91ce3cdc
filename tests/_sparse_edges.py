"""Input builders for the sparse-sender edge tests (plain numpy, no GPU).

The top-k senders select by key = |d| bits (csrc/choco_common.h): T is the k-th largest key,
every key above T is sent and the ties at T go to the lowest indices.  NaN keys sort above
inf, inf above FLT_MAX, subnormals below 2^23 and +-0 at 0, so a special value is an ordinary
key at an end of the key range -- where the sample window, the bucket geometry, the segmented
digits (20 / 9 / 0) and the warm windows do their arithmetic within a few keys of 0 or 2^31.
The families below put such keys where each of those pieces has to handle them.

Shapes (the smallest at which each path exists):
  FLAT_SIZES  4099 and 65536: the single-workgroup exact select and its upper edge kSmallN;
              65537: the first pipeline size (tiles of 32768 elements, the third holds one
              element); 163877 = 5 * 32768 + 37: six tiles, the last partial, and the 16384
              sampled elements cover a tenth of it.
  SEG_LAYOUT  the batched tile is 16384 elements: tensors one short of a tile, one tile, one
              over, a five-tile tensor, and tensors with k_s = 1.
  sample_runs the 64 runs of 256 elements that the flat pipeline's prologue samples, restated
              from the comment above load_sample (csrc/topk.hip): run j starts at
              4 * j * (((n - 256) // 63) >> 2).

A family is a function of (n, k, seed, computed) that returns a Case (x, xhat, memory, gamma):
  computed=False  the read-only form: xhat is None, the kernel sees the stored bits of x;
  computed=True   d = fl(x - xhat) is formed by the kernel (the xhat form), or
                  d = fl(x_new - xhat) after x_new = x + gamma (memory - xhat) (the gossip form).
"Placed" values sit at element 0 and n - 1 and on both sides of every tile edge (`tile`:
32768 flat, 16384 inside a segment); a segmented input applies a family per segment with the
segment's own k_s, so both ends of every segment are placed too.

  top_few        randn and 24 placed specials (+-inf, +-FLT_MAX, quiet NaNs of both signs):
                 fewer than the smallest k, so T stays finite and every special is selected.
  nan_flood      k + max(1, k // 2) NaNs: T is a NaN key and the tie quota is taken among NaNs.
                 Read-only: eight quiet payloads x both signs (the payload is part of the key,
                 equal payloads go to the lowest indices).  Computed: one payload, xhat finite.
                 placement "sampled" fills the sampled runs first, "hidden" keeps out of them.
  inf_flood      the same counts and placements with +-inf, and five NaNs: T = 0x7F800000.
  huge           every |d| in [2^126, FLT_MAX), distinct keys, and a tie cluster of more than
                 k / 2 elements at FLT_MAX.  Computed: x and xhat of opposite sign, and a few
                 positions where x - xhat overflows to +-inf.
  subnormal      every |d| < 2^-126 (keys below 2^23), -0 at every 7th element, 49 % non-zero:
                 T is subnormal at ratios 0.99 and 0.9 and 0 at 0.5.  Computed: d is the exact
                 difference of two normal numbers.
  zeros_few      k // 2 non-zero elements among +0 and -0: T = 0, ties to the lowest indices,
                 -0 sent with its sign.
  digit_edges    keys from {B - 1, B, B + 1}, B on a multiple of 2^20 or 2^9 (or, "span", in
                 the middle of one 512-key span): k // 2 keys B + 1, k keys B laid across the
                 first tile edge so that T = B and the quota of ties ends past that edge.
  inf_minus_inf  (computed only) 16 positions where d = inf - inf = NaN, with inf - finite,
                 finite - inf and NaN - finite next to them.

tests/test_sparse_edges_host.py holds the families to these claims.
"""
import zlib

import numpy as np

F32 = np.float32
U32 = np.uint32

FLAT_SIZES = [4099, 65536, 65537, 163877]
RATIOS = [0.99, 0.9, 0.5]
SEG_LAYOUT = [1, 3, 100, 16383, 16384, 16385, 40000, 70001]
SEG_N = sum(SEG_LAYOUT)
assert SEG_N == 159257
FLAT_TILE = 32768
SEG_TILE = 16384
SMALL_N = 65536
GAMMA = 0.9

KEY_INF = 0x7F800000
KEY_QNAN = 0x7FC00000
KEY_FLT_MAX = 0x7F7FFFFF
KEY_2P126 = 0x7E800000
KEY_MIN_NORMAL = 0x00800000
NAN_PAYLOADS = [0x000000, 0x000001, 0x000200, 0x0FFFFF, 0x100000, 0x155555, 0x2AAAAA, 0x3FFFFF]
DIGIT_BS = [0x00800000, 0x3F800000, 0x7F000000, 0x3F800200, 0x00000200, 0x7F7FFE00]
DIGIT_SPAN_B = 0x3F800100
N_SPECIAL = 24
N_INF_MINUS_INF = 16


def frozen(a):
    if a is not None:
        a.flags.writeable = False
    return a


def bounds(lens):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return list(zip(off[:-1].tolist(), off[1:].tolist()))


def sample_runs(n):
    """[(start, stop)] of the 64 sampled runs of 256 elements (n > 65536)."""
    stride = ((n - 256) // 63) >> 2
    return [(4 * j * stride, 4 * j * stride + 256) for j in range(64)]


def in_sample(n):
    m = np.zeros(n, dtype=bool)
    for a, b in sample_runs(n):
        m[a:b] = True
    return m


def placed(n, tile):
    """Element 0 and n - 1 and both sides of every tile edge."""
    pos = {0, n - 1}
    for t in range(tile, n, tile):
        pos.update((t - 1, t))
    return np.array(sorted(pos), dtype=np.int64)


def from_keys(keys, neg):
    """fp32 values with the given |v| bits and sign bits."""
    bits = np.asarray(keys, dtype=np.int64) | (np.asarray(neg, dtype=np.int64) << 31)
    return bits.astype(U32).view(F32)


def keys_of(d):
    return np.ascontiguousarray(d, dtype=F32).view(U32) & U32(0x7FFFFFFF)


def kth_key(d, k):
    """T: the k-th largest key."""
    kk = np.sort(keys_of(d))
    return int(kk[kk.size - k])


class Case:
    """One input: x, and in the computed form xhat, memory and gamma."""

    def __init__(self, x, xhat=None, memory=None, gamma=GAMMA):
        self.x, self.xhat, self.memory, self.gamma = frozen(x), frozen(xhat), frozen(memory), gamma

    def delta(self):
        """The delta of the read-only and xhat forms."""
        if self.xhat is None:
            return self.x
        with np.errstate(all="ignore"):
            return (self.x - self.xhat).astype(F32)

    def gossip(self):
        """(x_new, d) of the gossip form: three fp32 roundings (optim/utils.py:70-72), then
        d = fl(x_new - xhat)."""
        with np.errstate(all="ignore"):
            g = (F32(self.gamma) * (self.memory - self.xhat).astype(F32)).astype(F32)
            xn = (self.x + g).astype(F32)
            return xn, (xn - self.xhat).astype(F32)


def _rng(seed, *more):
    return np.random.default_rng([int(seed) & 0x7FFFFFFF, *[int(m) & 0x7FFFFFFF for m in more]])


def _spread(rng, n, count, tile, avoid=None):
    """`count` distinct positions: the placed ones first, then seeded ones."""
    count = min(count, n)
    free = np.ones(n, dtype=bool)
    if avoid is not None:
        free[avoid] = False
    first = [p for p in placed(n, tile).tolist() if free[p]][:count]
    free[first] = False
    rest = np.nonzero(free)[0]
    extra = rng.choice(rest, size=min(count - len(first), rest.size), replace=False)
    return np.concatenate([np.array(first, dtype=np.int64), extra.astype(np.int64)])


def _pair(rng, d, special, noisy_memory=True):
    """(x, xhat, memory) for the delta d.  At `special` positions fl(x - xhat) == d bit for bit:
    a non-finite d keeps x = d against a finite random xhat; a finite one has xhat = d, x = 2 d
    where 2 d is finite and d != 0, else xhat = +0, x = d.  Elsewhere xhat = randn / 2 and
    x = fl(d + xhat), so fl(x - xhat) is d to within a few ulps of x -- the tests' reference is
    fl(x - xhat) itself.  memory == xhat at the special positions (-0 where d is -0, so that
    the consensus step keeps x = -0) and, with noisy_memory, xhat + randn / 20 elsewhere."""
    n = d.size
    with np.errstate(all="ignore"):
        xhat = (rng.standard_normal(n) * 0.5).astype(F32)
        x = (d + xhat).astype(F32)
        d2 = (d + d).astype(F32)
    fin = np.isfinite(d)
    dbl = special & fin & np.isfinite(d2) & (d != 0)
    one = special & fin & ~dbl
    xhat[dbl], x[dbl] = d[dbl], d2[dbl]
    xhat[one], x[one] = F32(0), d[one]
    nf = special & ~fin
    x[nf] = d[nf]
    memory = xhat.copy()
    if noisy_memory:
        noise = (rng.standard_normal(n) * 0.05).astype(F32)
        memory[~special] = (xhat + noise)[~special]
    memory[special & (d == 0) & np.signbit(d)] = F32(-0.0)
    return x, xhat, memory


def _case(rng, d, special, computed, noisy_memory=True):
    if not computed:
        return Case(d)
    return Case(*_pair(rng, d, special, noisy_memory))


# ------------------------------------------------------------------------------ families
def top_few(n, k, seed, computed, tile=FLAT_TILE):
    rng = _rng(seed, n, 1)
    d = rng.standard_normal(n).astype(F32)
    pos = _spread(rng, n, N_SPECIAL, tile)
    kinds = [(KEY_INF, 0), (KEY_INF, 1), (KEY_FLT_MAX, 0), (KEY_FLT_MAX, 1), (KEY_QNAN, 0), (KEY_QNAN, 1)]
    kk = [kinds[i % 6] for i in range(pos.size)]
    d[pos] = from_keys([a for a, _ in kk], [b for _, b in kk])
    special = np.zeros(n, dtype=bool)
    special[pos] = True
    if not computed:
        return Case(d)
    x, xhat, memory = _pair(rng, d, special)
    # FLT_MAX as a computed difference: 2^127 - (-(2^127 - 2^104)), exact
    big = special & (keys_of(d) == KEY_FLT_MAX)
    sg = np.where(np.signbit(d[big]), F32(-1), F32(1))
    x[big] = sg * F32(2.0 ** 127)
    xhat[big] = -sg * F32(2.0 ** 127 - 2.0 ** 104)
    memory[big] = xhat[big]
    return Case(x, xhat, memory)


def flood_count(n, k):
    return min(n, k + max(1, k // 2))


def _flood_positions(rng, n, m, tile, placement):
    if placement is None:
        return _spread(rng, n, m, tile)
    ins = in_sample(n)
    inside, outside = np.nonzero(ins)[0], np.nonzero(~ins)[0]
    if placement == "sampled":
        a = rng.permutation(inside)[:m]
        b = rng.choice(outside, size=m - a.size, replace=False) if a.size < m else np.zeros(0, dtype=np.int64)
        return np.concatenate([a, b]).astype(np.int64)
    assert placement == "hidden" and m <= outside.size
    return rng.choice(outside, size=m, replace=False).astype(np.int64)


def nan_flood(n, k, seed, computed, tile=FLAT_TILE, placement=None):
    rng = _rng(seed, n, 2)
    d = rng.standard_normal(n).astype(F32)
    pos = _flood_positions(rng, n, flood_count(n, k), tile, placement)
    j = np.arange(pos.size)
    if computed:
        d[pos] = from_keys(np.full(pos.size, KEY_QNAN), np.zeros(pos.size, dtype=np.int64))
    else:
        d[pos] = from_keys(KEY_QNAN | np.array(NAN_PAYLOADS, dtype=np.int64)[j % 8], (j // 8) % 2)
    special = np.zeros(n, dtype=bool)
    special[pos] = True
    return _case(rng, d, special, computed)


def inf_flood(n, k, seed, computed, tile=FLAT_TILE, placement=None):
    rng = _rng(seed, n, 3)
    d = rng.standard_normal(n).astype(F32)
    pos = _flood_positions(rng, n, flood_count(n, k), tile, placement)
    d[pos] = from_keys(np.full(pos.size, KEY_INF), np.arange(pos.size) % 2)
    special = np.zeros(n, dtype=bool)
    special[pos] = True
    rest = np.nonzero(~special)[0]
    nans = rng.choice(rest, size=min(5, rest.size), replace=False)
    d[nans] = from_keys(np.full(nans.size, KEY_QNAN), np.arange(nans.size) % 2)
    special[nans] = True
    return _case(rng, d, special, computed)


def huge(n, k, seed, computed, tile=FLAT_TILE):
    rng = _rng(seed, n, 4)
    gap = max(1, (KEY_FLT_MAX - KEY_2P126) // n)
    kk = KEY_2P126 - 1 + np.cumsum(rng.integers(1, gap + 1, size=n))    # distinct, below FLT_MAX
    assert kk[-1] < KEY_FLT_MAX
    kk = rng.permutation(kk)
    cluster = _spread(rng, n, k // 2 + 1, tile)
    kk[cluster] = KEY_FLT_MAX
    d = from_keys(kk, rng.integers(0, 2, size=n))
    if not computed:
        return Case(d)
    with np.errstate(all="ignore"):
        x = (d * F32(0.5)).astype(F32)         # exact: |d| >= 2^126
        xhat = (-x).astype(F32)
    cl = np.zeros(n, dtype=bool)
    cl[cluster] = True
    sg = np.where(np.signbit(d[cl]), F32(-1), F32(1))
    x[cl] = sg * F32(2.0 ** 127)
    xhat[cl] = -sg * F32(2.0 ** 127 - 2.0 ** 104)
    over = _spread(rng, n, min(16, n // 8), tile, avoid=cluster)
    over = over[~cl[over]]
    sg = np.where(np.arange(over.size) % 2 == 1, F32(-1), F32(1))
    x[over] = sg * np.finfo(F32).max
    xhat[over] = -sg * np.finfo(F32).max
    return Case(x, xhat, xhat.copy())


def subnormal(n, k, seed, computed, tile=FLAT_TILE):
    rng = _rng(seed, n, 5)
    kk = np.zeros(n, dtype=np.int64)
    neg = np.zeros(n, dtype=np.int64)
    neg[::7] = 1                                                          # -0
    cand = np.nonzero(np.arange(n) % 7 != 0)[0]
    nz = rng.choice(cand, size=int(0.49 * n), replace=False)
    kk[nz] = rng.integers(1, KEY_MIN_NORMAL, size=nz.size)
    kk[nz[:4]] = [1, KEY_MIN_NORMAL - 1, 1, KEY_MIN_NORMAL - 1][:min(4, nz.size)]
    neg[nz] = rng.integers(0, 2, size=nz.size)
    d = from_keys(kk, neg)
    if not computed:
        return Case(d)
    # in units of 2^-149: xhat = s (2^23 + |m| + r), x = s (2^23 + r), d = x - xhat = -s |m|,
    # all three exact and x, xhat normal
    m = kk
    r = (rng.random(n) * (KEY_MIN_NORMAL - m)).astype(np.int64)
    s = np.where(neg == 1, 1, -1)              # d = -s |m| has the sign bit `neg`
    xhat = from_keys(KEY_MIN_NORMAL + m + r, s < 0)
    x = from_keys(KEY_MIN_NORMAL + r, s < 0)
    zero = kk == 0
    x[zero] = xhat[zero]                       # +0 = x - x
    mz = zero & (neg == 1)
    x[mz], xhat[mz] = F32(-0.0), F32(0.0)      # -0 = -0 - +0
    memory = xhat.copy()
    memory[mz] = F32(-0.0)
    return Case(x, xhat, memory)


def zeros_few(n, k, seed, computed, tile=FLAT_TILE):
    rng = _rng(seed, n, 6)
    d = from_keys(np.zeros(n, dtype=np.int64), rng.integers(0, 2, size=n))
    d[0] = F32(-0.0)
    nzpos = 1 + rng.choice(n - 1, size=min(k // 2, n - 1), replace=False) if n > 1 else np.zeros(0, dtype=np.int64)
    d[nzpos] = rng.standard_normal(nzpos.size).astype(F32)
    if not computed:
        return Case(d)
    special = (d == 0) & np.signbit(d)
    x, xhat, memory = _pair(rng, d, special)
    pz = (d == 0) & ~np.signbit(d)
    x[pz] = xhat[pz]                           # +0 = x - x, x != 0
    memory[pz] = xhat[pz]
    return Case(x, xhat, memory)


def digit_edges(n, k, seed, computed, tile=FLAT_TILE, B=DIGIT_BS[0]):
    rng = _rng(seed, n, 7, B)
    kk = np.full(n, B - 1, dtype=np.int64)
    a = min(k // 2, n)
    above = rng.choice(n, size=a, replace=False)
    kk[above] = B + 1
    free = np.nonzero(kk == B - 1)[0]
    r = k - a                                   # the quota of ties at T = B
    b = min(k, free.size)
    e = int(np.searchsorted(free, min(tile, n)))
    start = max(0, min(e - r // 2, free.size - b))
    kk[free[start:start + b]] = B
    d = from_keys(kk, rng.integers(0, 2, size=n))
    return _case(rng, d, np.ones(n, dtype=bool), computed, noisy_memory=False)


def inf_minus_inf(n, k, seed, computed=True, tile=FLAT_TILE):
    assert computed, "inf - inf exists only as a computed delta"
    rng = _rng(seed, n, 8)
    d = rng.standard_normal(n).astype(F32)
    x, xhat, memory = _pair(rng, d, np.zeros(n, dtype=bool))
    pos = _spread(rng, n, min(N_INF_MINUS_INF, max(1, n // 4)), tile)
    inf = F32(np.inf)
    taken = np.zeros(n, dtype=bool)
    taken[pos] = True
    for i, p in enumerate(pos.tolist()):
        sg = F32(-1) if i % 2 else F32(1)
        x[p], xhat[p] = sg * inf, sg * inf                               # inf - inf
        for q, kind in ((p - 1, 0), (p + 1, 1), (p + 2, 2)):
            if 0 <= q < n and not taken[q]:
                taken[q] = True
                if kind == 0:
                    x[q] = sg * inf                                      # inf - finite
                elif kind == 1:
                    xhat[q] = sg * inf                                   # finite - inf
                else:
                    x[q] = from_keys([KEY_QNAN], [i % 2])[0]             # NaN - finite
    memory[taken] = xhat[taken]
    return Case(x, xhat, memory)


# ------------------------------------------------------------------------------ the variants
FAMILIES = {"top_few": top_few, "nan_flood": nan_flood, "inf_flood": inf_flood, "huge": huge,
            "subnormal": subnormal, "zeros_few": zeros_few, "digit_edges": digit_edges,
            "inf_minus_inf": inf_minus_inf}
FIRST_SIX = ["top_few", "nan_flood", "inf_flood", "huge", "subnormal", "zeros_few"]
DIGIT_TAGS = [f"digit_edges-{B:08x}" for B in DIGIT_BS] + ["digit_edges-span"]
PLACED_TAGS = ["nan_flood-sampled", "nan_flood-hidden", "inf_flood-sampled", "inf_flood-hidden"]
BASE_TAGS = FIRST_SIX + DIGIT_TAGS + ["inf_minus_inf"]


def tags(n=None, ratio=None, computed=True):
    """The variants that exist at (n, ratio, computed).  The sampled / hidden placements need
    the sample (n > 65536) and are built at ratios 0.99 and 0.9; inf_minus_inf is computed only."""
    out = [t for t in BASE_TAGS if computed or t != "inf_minus_inf"]
    if n is not None and n > SMALL_N and ratio in (0.99, 0.9):
        out += PLACED_TAGS
    return out


def digit_B(tag):
    return DIGIT_SPAN_B if tag.endswith("span") else int(tag.split("-")[1], 16)


def build(tag, n, k, computed, tile=FLAT_TILE, seed=None):
    """The Case of variant `tag` (a family name, a placement or a digit_edges B)."""
    seed = zlib.crc32(tag.encode()) if seed is None else seed
    name, _, arg = tag.partition("-")
    if name == "digit_edges":
        return digit_edges(n, k, seed, computed, tile=tile, B=digit_B(tag))
    if arg:
        return FAMILIES[name](n, k, seed, computed, tile=tile, placement=arg)
    return FAMILIES[name](n, k, seed, computed, tile=tile)


def _whole(n, keys, neg, computed, rng):
    d = from_keys(keys, neg)
    return _case(rng, d, np.ones(n, dtype=bool), computed, noisy_memory=False)


def _mixed_segment(s, m, k, computed):
    """`mixed`: one family per tensor in turn, with a lone NaN, a whole tensor of +-0, of NaN
    and of +-inf among them."""
    rng = _rng(991, s, m)
    j = np.arange(m)
    if s == 0:                                                   # the length-1 tensor: a NaN
        return _whole(m, np.full(m, KEY_QNAN), j % 2, computed, rng)
    if s == 2:
        return _whole(m, np.zeros(m, dtype=np.int64), rng.integers(0, 2, size=m), computed, rng)
    if s == 3:
        pay = np.array(NAN_PAYLOADS, dtype=np.int64)[rng.integers(0, 8, size=m)]
        return _whole(m, KEY_QNAN | (0 if computed else pay), j % 2, computed, rng)
    if s == 4:
        return _whole(m, np.full(m, KEY_INF), rng.integers(0, 2, size=m), computed, rng)
    tag = {1: "top_few", 5: "digit_edges-3f800000", 6: "subnormal", 7: "huge"}[s]
    return build(tag, m, k, computed, tile=SEG_TILE, seed=991 + s)


def topk_k(n, ratio):
    return max(1, int(n * (1 - ratio)))


def segmented(tag, ratio, computed, lens=SEG_LAYOUT):
    """Variant `tag` (or "mixed") applied per tensor with the tensor's own k_s."""
    parts = []
    for s, m in enumerate(lens):
        k = topk_k(m, ratio)
        if tag == "mixed":
            parts.append(_mixed_segment(s, m, k, computed))
        else:
            parts.append(build(tag, m, k, computed, tile=SEG_TILE, seed=zlib.crc32(tag.encode()) + 17 * s))
    x = np.concatenate([p.x for p in parts])
    if not computed:
        return Case(x)
    return Case(x, np.concatenate([p.xhat for p in parts]), np.concatenate([p.memory for p in parts]))


def seg_tags(computed=True):
    return tags(computed=computed) + ["mixed"]


def randn_case(n, seed, computed):
    """An ordinary input (the calls between the special ones of a warm sequence)."""
    rng = _rng(seed, n, 9)
    d = rng.standard_normal(n).astype(F32)
    return _case(rng, d, np.zeros(n, dtype=bool), computed)


WARM_SEQUENCE = ["randn", "randn", "top_few", "randn", "nan_flood", "randn", "inf_flood", "subnormal", "zeros_few",
                 "randn", "huge", "digit_edges-3f800000", "randn", "randn"]
