"""GPU parity of the RECEIVER kernels against the numpy oracle: the QSGD decode / accumulate /
range accumulate / extrapolate / fused receive at every container width, the sign receiver
in its two-rounding and ECD modes, the DeepSqueeze local decode and the sparse extrapolate.

Every message is made on the host by the oracle (O.qsgd_pack from chosen levels, O.sign_pack,
chosen norms) and uploaded, so a failure points at the receiver and every QSGD message holds
level 0 and the top level 2^q - 1.  The reference is the oracle alone, never another entry
point of the library, and the comparison is same_bits on the whole buffer (the fused
receive's norms: rtol 1e-6 against the fp64 norm of the oracle's own x_new - x_hat_new, the
bound test_qsgd_segmented_layout_norms_and_levels uses for device norms).
Run on an MI355X with `pytest -m gpu`."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import same_bits
from oracle import choco_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the shared inputs are read-only)


def host(t):
    return t.cpu().numpy()


def randn(n, seed, scale=1.0):
    """Host fp32 normals (every input here is generated on the host from a seed)."""
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(F32)


def seg_table(lens):
    return dev(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)) if len(lens) > 1 else None


def frozen(a):
    a.flags.writeable = False
    return a


def weights_for(nmsg):
    """Not all equal, a negative one (DeepSqueeze's self weight is negative) and 1.0."""
    return {1: [-0.75], 3: [1 / 3, -0.5, 1.0], 8: [1 / 3, -0.5, 1.0, 0.125, 0.3, 0.7, -1.0, 0.2]}[nmsg]


def bounds(lens):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return list(zip(off[:-1].tolist(), off[1:].tolist()))


# ------------------------------------------------------------------------------------ QSGD
# Granules: 8-element groups, 2048-element decode tiles, 4096-element fused-receive tiles,
# 8192-element range granules.  18,445 = 2 * 8192 + 2048 + 13: three ranges (the last partial),
# ten decode tiles (the last: one full group and a 5-element group), a fused-receive tile
# whose second group is mostly absent.  "ragged": boundaries on a tile edge (2048), mid-group
# (2049, 2056), on a range granule (8192), one past a granule (16385) and just before the
# partial tail (18432).  "tiny": 300 tensors of 1-13 elements between larger ones.
QN = 18_445
QLAYOUTS = {
    "flat": [QN],
    "ragged": [3, 2045, 1, 7, 6136, 8193, 2047, 13],
    "tiny": [3_000] + [1 + (i * 7) % 13 for i in range(300)] + [20_011],
    "n5": [5], "n8": [8], "n2048": [2048], "n2049": [2049],
}
assert sum(QLAYOUTS["ragged"]) == QN
ALL_Q = [1, 2, 3, 4, 5, 8, 9, 16]
ZERO_SEG = 4  # the zero-norm case: this segment of the self message


def _qid(c):
    q, layout, nmsg, biased, zero = c
    return f"q{q}-{layout}-m{nmsg}" + ("-biased" if biased else "") + ("-zeronorm" if zero else "")


# (q, layout, messages, is_biased, zero norm)
QCASES = [(q, lay, 3, False, False) for q in ALL_Q for lay in ("flat", "ragged")]
QCASES += [(q, lay, m, False, False) for q in (2, 16) for m in (1, 8) for lay in ("flat", "ragged")]
QCASES += [(3, "ragged", 3, True, False), (8, "ragged", 3, True, False)]
QCASES += [(4, "tiny", 3, False, False), (9, "tiny", 3, True, False), (1, "tiny", 8, False, False)]
QCASES += [(4, "ragged", 3, False, True)]
QCASES += [(q, lay, 3, False, False) for lay in ("n5", "n8", "n2048", "n2049") for q in (1, 4, 16)]
# the single-message entry points: the same q and layouts, message 0 (the zero-norm one: the self message)
QSINGLE = [c for c in QCASES if c[2] == 3]


@functools.lru_cache(maxsize=None)
def qcase(q, layout, nmsg, biased, zero):
    """Inputs and oracle results of one case, computed once and shared (read-only)."""
    lens = QLAYOUTS[layout]
    n, s = sum(lens), 2 ** q - 1
    segs = bounds(lens)
    firsts = np.array([a for a, _ in segs])
    lasts = np.array([b - 1 for _, b in segs])
    rng = np.random.default_rng([q, n, len(lens), nmsg, int(biased), int(zero)])
    w = weights_for(nmsg)
    slot = nmsg // 2
    msgs = []
    for m in range(nmsg):
        lvl = rng.integers(0, s + 1, size=n)
        # level 0 and the top level in every message: at each tensor's first and last element
        # (which one where alternates by message), so also at the buffer's ends
        lo, hi = (0, s) if m % 2 == 0 else (s, 0)
        lvl[lasts] = hi
        lvl[firsts] = lo
        lvl[n - 1], lvl[n - 2], lvl[1], lvl[0] = hi, lo, hi, lo
        d = rng.standard_normal(n).astype(F32)  # its signs are the message's sign plane
        norms = rng.uniform(0.5, 4.0, size=len(lens)).astype(F32)
        if zero and m == slot:
            norms[ZERO_SEG] = 0.0
        packed = O.qsgd_pack(lvl.astype(F32), d, q)
        levels, neg = O.qsgd_unpack(packed, n, q)
        assert np.array_equal(levels.astype(np.int64), lvl) and levels.min() == 0 and levels.max() == s
        dec = np.concatenate([O.qsgd_decode(levels[a:b], neg[a:b], norms[i], s, b - a, is_biased=biased)
                              for i, (a, b) in enumerate(segs)])
        msgs.append(SimpleNamespace(lvl=frozen(lvl), d=frozen(d), norms=frozen(norms), packed=frozen(packed),
                                    dec=frozen(dec)))
    x0, hat0, mem0 = (frozen(rng.standard_normal(n).astype(F32)) for _ in range(3))
    hat1, mem1 = hat0.copy(), mem0.copy()
    with np.errstate(invalid="ignore"):
        O.qsgd_accumulate(hat1, mem1, [m.dec for m in msgs], w, slot)
    nan_at = np.zeros(n, dtype=bool)
    if zero:
        nan_at[segs[ZERO_SEG][0]:segs[ZERO_SEG][1]] = True
    assert np.array_equal(np.isnan(mem1), nan_at) and np.array_equal(np.isnan(hat1), nan_at)
    return SimpleNamespace(q=q, lens=lens, n=n, nseg=len(lens), biased=biased, zero=zero, w=w, slot=slot, msgs=msgs,
                           segs=segs, x0=x0, hat0=hat0, mem0=mem0, hat1=frozen(hat1), mem1=frozen(mem1),
                           nan_at=frozen(nan_at), single=slot if zero else 0)


def upload(c):
    return [(dev(m.packed), dev(m.norms)) for m in c.msgs]


def agrees(got, want, nan_at):
    """NaN at exactly the oracle's NaN positions, identical bits everywhere else."""
    got = host(got) if isinstance(got, torch.Tensor) else got
    return np.array_equal(np.isnan(got), nan_at) and np.array_equal(np.isnan(want), nan_at) and same_bits(got, want)


@pytest.mark.parametrize("case", QSINGLE, ids=_qid)
def test_qsgd_decode_vs_oracle(case):
    from chocosgd_amd import codec
    c = qcase(*case)
    m = c.msgs[c.single]
    out = codec.qsgd_decode(dev(m.packed), dev(m.norms), c.n, c.q, is_biased=c.biased, seg_off=seg_table(c.lens),
                            nseg=c.nseg)
    assert agrees(out, m.dec, c.nan_at)


@pytest.mark.parametrize("case", QSINGLE, ids=_qid)
def test_qsgd_extrapolate_vs_oracle(case):
    """ECD's replica update fmaf(b, decode(m), target * a) with (a, b) = (1 - 2/t, 2/t)."""
    from chocosgd_amd import codec
    c = qcase(*case)
    m = c.msgs[c.single]
    packed, norms, so = dev(m.packed), dev(m.norms), seg_table(c.lens)
    for t in (2, 3, 1000):
        a, b = O.ecd_coeffs(t)
        target = dev(c.mem0)
        codec.qsgd_extrapolate(packed, norms, c.n, c.q, target, float(a), float(b), is_biased=c.biased, seg_off=so,
                               nseg=c.nseg)
        with np.errstate(invalid="ignore"):
            want = O.ecd_extrapolate(c.mem0, m.dec, t)
        assert agrees(target, want, c.nan_at), t


@pytest.mark.parametrize("with_self", [True, False], ids=["self", "noself"])
@pytest.mark.parametrize("case", QCASES, ids=_qid)
def test_qsgd_accumulate_vs_oracle(case, with_self):
    """x_hat += q_self at a middle slot, memory += w * q per message in order (two roundings);
    without a self message x_hat is not passed and memory is the same."""
    from chocosgd_amd import codec
    c = qcase(*case)
    hat, mem = dev(c.hat0), dev(c.mem0)
    codec.qsgd_accumulate(upload(c), c.w, c.slot if with_self else -1, c.n, c.q, mem,
                          xhat_self=hat if with_self else None, is_biased=c.biased, seg_off=seg_table(c.lens),
                          nseg=c.nseg)
    assert agrees(mem, c.mem1, c.nan_at)
    if with_self:
        assert agrees(hat, c.hat1, c.nan_at)
    else:
        assert same_bits(host(hat), c.hat0)


@pytest.mark.parametrize("case", QCASES, ids=_qid)
def test_qsgd_accumulate_range_vs_oracle(case):
    """The chunked wire's receive: each range a self-contained message O.qsgd_pack(lvl[e0:e1],
    d[e0:e1], q) (the library rebases its plane pointers to absolute groups).  After the first
    range only, elements >= e1 are untouched; after all ranges x_hat / memory are the oracle's
    whole-buffer result."""
    from chocosgd_amd import codec
    c = qcase(*case)
    ranges = codec.qsgd_chunks(c.n, 3)
    assert ranges[0][0] == 0 and ranges[-1][1] == c.n and (c.n != QN or len(ranges) == 3)
    hat, mem, so = dev(c.hat0), dev(c.mem0), seg_table(c.lens)
    norms = [dev(m.norms) for m in c.msgs]
    for i, (e0, e1) in enumerate(ranges):
        part = [(dev(O.qsgd_pack(m.lvl[e0:e1].astype(F32), m.d[e0:e1], c.q)), nm) for m, nm in zip(c.msgs, norms)]
        codec.qsgd_accumulate_range(part, c.w, c.slot, c.n, c.q, mem, e0, e1, xhat_self=hat, is_biased=c.biased,
                                    seg_off=so, nseg=c.nseg)
        if i == 0:
            h, m_ = host(hat), host(mem)
            assert same_bits(h[e1:], c.hat0[e1:]) and same_bits(m_[e1:], c.mem0[e1:])
            assert agrees(h[:e1], c.hat1[:e1], c.nan_at[:e1]) and agrees(m_[:e1], c.mem1[:e1], c.nan_at[:e1])
    assert agrees(hat, c.hat1, c.nan_at)
    assert agrees(mem, c.mem1, c.nan_at)


@pytest.mark.parametrize("case", QCASES, ids=_qid)
def test_qsgd_recv_gossip_norms_vs_oracle(case):
    """The fused receive + consensus step + norm pass, twice in a row on the same workspace: a
    ticket or accumulator left dirty by the first call shows in the second call's norms."""
    from chocosgd_amd import codec
    c = qcase(*case)
    gamma = 0.37
    x, hat, mem, so = dev(c.x0), dev(c.hat0), dev(c.mem0), seg_table(c.lens)
    msgs = upload(c)
    xo, ho, mo = c.x0.copy(), c.hat0.copy(), c.mem0.copy()
    for rep in range(2):
        norms = codec.qsgd_recv_gossip_norms(msgs, c.w, c.slot, x, mem, hat, gamma, c.q, is_biased=c.biased,
                                             seg_off=so, nseg=c.nseg)
        with np.errstate(invalid="ignore"):
            O.qsgd_accumulate(ho, mo, [m.dec for m in c.msgs], c.w, c.slot)
            xo = O.gossip_step(xo, mo, ho, gamma)
            want = O.l2_norms(xo - ho, c.lens)  # fp64 sums of the oracle's own x_new - x_hat_new
        assert agrees(hat, ho, c.nan_at), rep
        assert agrees(mem, mo, c.nan_at), rep
        assert agrees(x, xo, c.nan_at), rep
        got = host(norms)
        nan_seg = np.arange(c.nseg) == ZERO_SEG if c.zero else np.zeros(c.nseg, dtype=bool)
        print(f"rep {rep}: max relative norm error {np.nanmax(np.abs(got / want - 1)):.3g}")
        assert np.array_equal(np.isnan(got), nan_seg) and np.array_equal(np.isnan(want), nan_seg), rep
        assert np.allclose(got[~nan_seg], want[~nan_seg], rtol=1e-6, atol=0), rep


# ------------------------------------------------------------------------------------ sign
# The receiver works on the (32, N') view in 1024-column blocks of four 256-column waves.
# n in {1, 33, 1000}: one partial column block.  70,001: N' = 2188, every row start 16-byte
# aligned; 70,035: N' = 2189, row starts cycle through all four misalignments (lane 0 / lane
# 63 realignment); both have interior waves and a third, partial column block.  "ragged":
# rows wholly inside the 40,000-element tensor next to rows that straddle several; "many":
# thousands of tensors of 1-39 elements (every row straddles).
SN = 70_035


def _many(n):
    lens, tot = [], 0
    for m in np.random.default_rng(11).integers(1, 40, size=n).tolist():
        m = min(m, n - tot)
        lens.append(m)
        tot += m
        if tot == n:
            return lens


SLAYOUTS = {
    "n1": [1], "n33": [33], "n1000": [1000], "n70001": [70_001],
    "flat": [SN], "ragged": [3, 40_000, 5, 17, 30_010], "many": _many(SN),
}
assert all(sum(SLAYOUTS[k]) == SN for k in ("flat", "ragged", "many")) and len(SLAYOUTS["many"]) > 3000
SCASES = [(lay, 3) for lay in SLAYOUTS] + [(lay, m) for lay in ("n33", "n70001", "ragged") for m in (1, 8)]


@functools.lru_cache(maxsize=None)
def scase(layout, nmsg):
    lens = SLAYOUTS[layout]
    n = sum(lens)
    rng = np.random.default_rng([n, len(lens), nmsg])
    msgs = []
    for _ in range(nmsg):
        words = O.sign_pack(rng.standard_normal(n).astype(F32))
        # L1-like norms: norm / numel of order one, so that w * (norm / numel) rounds visibly
        norms = (rng.uniform(0.2, 2.0, size=len(lens)) * np.array(lens)).astype(F32)
        msgs.append((frozen(words), frozen(norms)))
    return SimpleNamespace(lens=lens, n=n, nseg=len(lens), msgs=msgs, w=weights_for(nmsg),
                           t0=frozen(rng.standard_normal(n).astype(F32)))


@pytest.mark.parametrize("two_roundings", [False, True], ids=["fma", "two_roundings"])
@pytest.mark.parametrize("layout,nmsg", SCASES)
def test_sign_axpy_vs_oracle(layout, nmsg, two_roundings):
    """target += w_m * (norm_s / numel_s * sign) message by message in order: torch's
    add_(u, alpha=w) (one rounding, DCD) or add_(w * u) (two, DeepSqueeze)."""
    from chocosgd_amd import codec
    c = scase(layout, nmsg)
    target = dev(c.t0)
    codec.sign_axpy([(dev(p), dev(nm)) for p, nm in c.msgs], c.w, c.n, target, seg_off=seg_table(c.lens),
                    nseg=c.nseg, two_roundings=two_roundings)
    want = c.t0.copy()
    for (words, norms), w in zip(c.msgs, c.w):
        O.sign_axpy(want, words, norms, c.lens, w, two_roundings)
    assert same_bits(host(target), want)


@pytest.mark.parametrize("layout", list(SLAYOUTS))
def test_sign_extrapolate_vs_oracle(layout):
    """ECD: target_s = (target_s * a) + ((b * norm_s) / numel_s) * sign, (a, b) = (1 - 2/t, 2/t)."""
    from chocosgd_amd import codec
    c = scase(layout, 3)
    words, norms = c.msgs[0]
    dw, dn, so = dev(words), dev(norms), seg_table(c.lens)
    for t in (2, 3, 1000):
        a, b = O.ecd_coeffs(t)
        target = dev(c.t0)
        codec.sign_extrapolate(dw, dn, c.n, target, float(a), float(b), seg_off=so, nseg=c.nseg)
        assert same_bits(host(target), O.ecd_sign_extrapolate(c.t0, words, norms, c.lens, t)), t


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, 1e-41, -1e-41, np.nan], dtype=F32)  # 1e-41: subnormal
LLAYOUTS = {"n1023": [1023], "n1024": [1024], "n1025": [1025], "flat": SLAYOUTS["flat"],
            "ragged": SLAYOUTS["ragged"], "many": SLAYOUTS["many"]}


def local_input(lens):
    """Normals with 0.0, -0.0, +-inf, subnormals and NaN as tensors' first and last elements
    and inside tensors."""
    n = sum(lens)
    segs = bounds(lens)
    x = randn(n, n + len(lens))
    k = 0
    for a, b in segs[::max(1, len(segs) // 40)]:
        for p in sorted({a, (a + b) // 2, b - 1}):
            x[p] = SPECIALS[k % len(SPECIALS)]
            k += 1
    a, b = max(segs, key=lambda ab: ab[1] - ab[0])
    p = a + (b - a) // 3
    x[p:p + len(SPECIALS)] = SPECIALS                          # all of them inside the largest tensor
    x[0] = x[n - 1] = np.nan                                   # the buffer's first and last element
    if len(segs) > 2:
        x[segs[1][0]] = x[segs[-2][1] - 1] = np.nan            # a tensor's first / last element inside the buffer
    return x


@pytest.mark.parametrize("layout", list(LLAYOUTS))
def test_sign_local_decode_vs_oracle(layout):
    """(norm_s * torch.sign(x)) / numel_s with torch.sign's values: +-0 and NaN give 0."""
    from chocosgd_amd import codec
    lens = LLAYOUTS[layout]
    x = local_input(lens)
    assert np.isnan(x).sum() >= 3 and np.isinf(x).any() and (x == 0).any()
    norms = (np.random.default_rng(len(lens)).uniform(0.2, 2.0, size=len(lens)) * np.array(lens)).astype(F32)
    out = codec.sign_local_decode(dev(x), dev(norms), seg_off=seg_table(lens), nseg=len(lens))
    want = O.sign_local(x, norms, lens)
    assert not np.isnan(want).any()
    got = host(out)
    assert not np.isnan(got).any(), f"NaN at {np.nonzero(np.isnan(got))[0][:8]}: torch.sign(NaN) is 0"
    assert same_bits(got, want)


def test_sign_local_decode_one_element():
    from chocosgd_amd import codec
    norms = np.array([3.0], dtype=F32)
    for v in SPECIALS.tolist() + [2.5, -2.5]:
        x = np.array([v], dtype=F32)
        out = codec.sign_local_decode(dev(x), dev(norms))
        assert same_bits(host(out), O.sign_local(x, norms, [1])), v


# ------------------------------------------------------------------------------------ sparse
SPN = 20_011


def _sparse(view, k, seed):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(SPN).astype(F32)
    n = SPN - view
    idx = np.sort(rng.choice(n, size=k, replace=False)).astype(np.int32)
    return base, n, idx, rng.standard_normal(k).astype(F32)


@pytest.mark.parametrize("k", [1, 257, 5000])
@pytest.mark.parametrize("view", [0, 1], ids=["whole", "view1"])
def test_sparse_extrapolate_vs_oracle(view, k):
    """target[idx] = fmaf(b, v, target[idx] * a) on the buffer and on its [1:] view (4-byte
    aligned only); everything outside idx, the element in front of the view included, keeps
    its bits."""
    from chocosgd_amd import codec
    base, n, idx, vals = _sparse(view, k, 100 * k + view)
    a, b = O.ecd_coeffs(3)
    buf = dev(base)
    codec.sparse_extrapolate(dev(vals), dev(idx), buf[view:], float(a), float(b))
    want = base.copy()
    want[view:][idx] = O.fma32(b, vals, (base[view:][idx] * a).astype(F32))
    assert same_bits(host(buf), want)


def test_sparse_extrapolate_bad_indices_skipped_and_counted():
    """An index of -1 and one of n: both skipped, the rest applied, and the guard raises."""
    from chocosgd_amd import codec
    base, n, idx, vals = _sparse(0, 257, 7)
    idx = idx.copy()
    idx[0], idx[-1] = -1, n
    ok = slice(1, -1)
    a, b = O.ecd_coeffs(1000)
    guard = codec.IndexGuard(torch.device(DEV))
    buf = dev(base)
    codec.sparse_extrapolate(dev(vals), dev(idx), buf, float(a), float(b), guard=guard)
    want = base.copy()
    want[idx[ok]] = O.fma32(b, vals[ok], (base[idx[ok]] * a).astype(F32))
    assert same_bits(host(buf), want)
    guard.arm()
    with pytest.raises(RuntimeError, match="out of range"):
        guard.check(wait=True)
    assert guard.reported == 2
