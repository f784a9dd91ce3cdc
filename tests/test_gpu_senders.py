"""GPU parity of the SENDER kernels against the numpy oracle where they can be subtly wrong:
the QSGD quantize at the edges of its fast division's guard (csrc/qsgd.hip QDiv: norm in
[2^-30, 2^96], first quotient in [2^-60, 2^7], taken per 8-element group and per wave), at
every q from 1 to 16, across tensor boundaries inside a tile, as chunked ranges, with device
norms at extreme scales; and the QSGD and sign senders on NaN, +-inf, -0 and subnormal deltas,
including that the self-resetting fp64 norm accumulators are clean after a call that summed
inf or NaN.

Inputs come from tests/_sender_edges.py (tests/test_sender_edges_host.py holds them to their
coverage and pins the oracle's division to exact rationals).  The reference is the oracle
alone: wires and words by np.array_equal (padding included), floats by same_bits, device norms
equal or adjacent to the oracle's fp32 value (both sides sum at most 65,573 terms that are
exact in fp64, so they agree to ~2^-37 before the one rounding to fp32, which is monotone),
with 0, inf and NaN matching as classes.  Run on an MI355X with `pytest -m gpu`."""
import functools

import numpy as np
import pytest
import torch

import _sender_edges as E
from conftest import same_bits
from oracle import choco_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
SN = E.SN
GAMMA = 0.37


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV) if a is not None else None  # (a copy: shared inputs are read-only)


def host(t):
    return t.cpu().numpy()


def seg_table(lens):
    return dev(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)) if len(lens) > 1 else None


@functools.lru_cache(maxsize=None)
def device_uniforms(n, seed, offset):
    return E.frozen(O.qsgd_uniforms(n, seed, offset))


@functools.lru_cache(maxsize=None)
def pinned_uniforms(n, seed):
    return E.frozen(E.uniforms(n, seed))


def agrees(got, want):
    """NaN at exactly the oracle's positions, identical bits everywhere else."""
    return np.array_equal(np.isnan(got), np.isnan(want)) and same_bits(got, want)


def oracle_message(d, lens, norms, q, biased, u):
    """(levels, wire, dense, decode of the wire) of the delta d, per tensor with its norm."""
    s = 2 ** q - 1
    segs = E.bounds(lens)
    with np.errstate(all="ignore"):
        lvl = np.concatenate([O.qsgd_levels(d[a:b], s, u[a:b], norms[i]) for i, (a, b) in enumerate(segs)])
        wire = O.qsgd_pack(lvl, d, q)
        dense = np.concatenate([O.qsgd_dense(d[a:b], s, u[a:b], norms[i], is_biased=biased)
                                for i, (a, b) in enumerate(segs)])
        levels, neg = O.qsgd_unpack(wire, d.size, q)
        dec = np.concatenate([O.qsgd_decode(levels[a:b], neg[a:b], norms[i], s, b - a, is_biased=biased)
                              for i, (a, b) in enumerate(segs)])
    return lvl, wire, dense, dec


def check_message(packed, norms_dev, dense, d, lens, norms, q, biased, u):
    """The three assertions of every QSGD case: the whole wire, dense_out, the library's
    decode of its own wire against the oracle's decode of the oracle's wire."""
    from chocosgd_amd import codec
    lvl, wire, want_dense, want_dec = oracle_message(d, lens, norms, q, biased, u)
    got = host(packed)
    bad = np.nonzero(got != wire)[0]
    assert bad.size == 0, f"{bad.size} wire bytes differ, first at {bad[:8]}"
    gd = host(dense)
    diff = np.nonzero(~(np.isnan(gd) & np.isnan(want_dense)) & (gd.view(np.uint32) != want_dense.view(np.uint32)))[0]
    assert diff.size == 0, f"{diff.size} dense values differ, first at {diff[:8]}: d {d[diff[:4]]} got " \
                           f"{gd[diff[:4]]} want {want_dense[diff[:4]]}"
    assert agrees(gd, want_dense)
    dec = codec.qsgd_decode(packed, norms_dev, d.size, q, is_biased=biased, seg_off=seg_table(lens), nseg=len(lens))
    assert agrees(host(dec), want_dec)
    return lvl


def pinned_case(x, xhat, lens, norms, q, biased, pin_u, seed=0x5EED, offset=3):
    """qsgd_compress with pinned norms; the uniforms pinned (u_in: the sharp ones, under which
    the level shows the last bit of the quotient) or the device stream's."""
    from chocosgd_amd import codec
    n = x.size
    norms = np.asarray(norms, dtype=F32)
    u = E.sharp_uniforms(E.delta_of(x, xhat), lens, norms, 2 ** q - 1, seed) if pin_u else \
        device_uniforms(n, seed, offset)
    packed, nout, dense = codec.qsgd_compress(dev(x), q, is_biased=biased, xhat=dev(xhat), seg_off=seg_table(lens),
                                              nseg=len(lens), norm_in=dev(norms), u_in=dev(u) if pin_u else None,
                                              seed=seed, offset=offset, want_dense=True)
    assert same_bits(host(nout), norms)
    return check_message(packed, nout, dense, E.delta_of(x, xhat), lens, norms, q, biased, u)


# ------------------------------------------------------------------ A. the guard, pinned norm
PINNED = {
    "2^-30": F32(2.0 ** -30), "prev(2^-30)": E.prev32(F32(2.0 ** -30)), "2^96": F32(2.0 ** 96),
    "next(2^96)": E.next32(F32(2.0 ** 96)), "1": F32(1.0), "0x1.fffffep+0": E.prev32(F32(2.0)), "3e-5": F32(3e-5),
    "2^-126": F32(2.0 ** -126), "2^-140": F32(2.0 ** -140), "FLT_MAX": np.finfo(F32).max, "inf": F32(np.inf),
    "nan": F32(np.nan), "0": F32(0.0),
    # out of range, no power of two, and T_lo = 2^-60 norm still representable: only the norm
    # range of the guard keeps the fast form away from quotients whose residual underflows (an
    # exact emulation of the fast form is off by an ulp on some ladder values at this norm; at
    # 2^-126 1 / norm is exact, and below 2^-90 T_lo is 0 and flags every nonzero value)
    "1.7*2^-80": F32(1.7 * 2.0 ** -80),
}
GUARD_CASES = [(name, q, with_xhat, (i + j + int(with_xhat)) % 2 == 0, False)
               for i, name in enumerate(PINNED) for j, q in enumerate((1, 4, 8, 16)) for with_xhat in (False, True)]
GUARD_CASES.append(("3e-5", 4, True, True, True))   # (norm, q, xhat, pinned uniforms, biased)
GUARD_CASES.append(("1", 16, False, False, True))


def _gid(c):
    name, q, with_xhat, pin_u, biased = c
    return f"N={name}-q{q}-" + ("xhat" if with_xhat else "plain") + ("-uin" if pin_u else "-stream") + \
        ("-biased" if biased else "")


def guard_input(name, q, with_xhat):
    d, is_ladder = E.pinned_delta(PINNED[name], 2 ** q - 1)
    return E.under_xhat(d, is_ladder) if with_xhat else (d, None)


@pytest.mark.parametrize("case", GUARD_CASES, ids=_gid)
def test_qsgd_guard_pinned_norm(case):
    """Values a few ulps on both sides of t = T_lo and q0 = 128, the top level and the clamp
    above it, and NaN, +-inf, +-0 and subnormals, in waves with no, some and only flagged
    groups (full tiles) and in the partial tile.  Without x_hat: the 512-thread kernel, with
    it the 256-thread one.  Out-of-range norms (also 0, inf, NaN): everything takes the IEEE
    division and must match all the same."""
    name, q, with_xhat, pin_u, biased = case
    x, xhat = guard_input(name, q, with_xhat)
    lvl = pinned_case(x, xhat, [SN], [PINNED[name]], q, biased, pin_u)
    if F32(2.0 ** -30) <= PINNED[name] <= F32(2.0 ** 96):  # (NaN compares false)
        s = 2 ** q - 1
        assert (lvl == s).any() and (lvl > s).any() and np.isnan(lvl).any()  # top level, clamp, NaN -> 0


# ------------------------------------------------------------------ B. every q
@pytest.mark.parametrize("q", list(range(1, 17)))
def test_qsgd_every_q(q):
    """q = 5, 6, 7 and 9..15 (container wider than q) through the quantize too."""
    x, _ = guard_input("1", q, False)
    pinned_case(x, None, [SN], [F32(1.0)], q, False, False, seed=0xABCDE + q, offset=q)


# ------------------------------------------------------------------ C. segment switches
RAGGED = E.QLAYOUTS["ragged"]
# "far": out-of-range norms at which the fast form's residual underflows while T_lo is still
# representable -- a fast quotient kept for them (a guard left over from the previous tensor)
# is wrong by an ulp on some values, which it is not one step outside the range as in "near"
RAGGED_NORMS = {
    "near": np.array([1.0, E.prev32(F32(2.0 ** -30)), 2.0 ** 96, 3e-5, 0.0], dtype=F32),
    "far": np.array([3e-5, 1.7 * 2.0 ** -80, 1.0, 1.3 * 2.0 ** -89, 0.0], dtype=F32),
}
SEG_CASES = [(4, False, True, False), (4, True, False, False), (16, False, False, False), (16, True, True, False),
             (4, True, True, True)]  # (q, xhat, pinned uniforms, biased)


def ragged_input(q, with_xhat, which="near"):
    d, is_ladder = E.ragged_delta(RAGGED_NORMS[which], 2 ** q - 1)
    return E.under_xhat(d, is_ladder) if with_xhat else (d, None)


@pytest.mark.parametrize("which", list(RAGGED_NORMS))
@pytest.mark.parametrize("q,with_xhat,pin_u,biased", SEG_CASES)
def test_qsgd_segment_switches_pinned_norms(q, with_xhat, pin_u, biased, which):
    """Every full tile crosses a tensor boundary and a thread's groups change tensor between
    steps: an in-range norm after an out-of-range one and the other way round (a stale guard
    would keep or lose the fast form), a group straddling a boundary, a zero-norm tensor."""
    x, xhat = ragged_input(q, with_xhat, which)
    d = E.delta_of(x, xhat)
    norms = RAGGED_NORMS[which]
    pinned_case(x, xhat, RAGGED, norms, q, biased, pin_u)
    # the zero-norm tensor: NaN in the oracle's dense at all its positions, and only NaN from
    # norms or deltas elsewhere (what check_message compared position by position)
    _, _, dense, dec = oracle_message(d, RAGGED, norms, q, biased, pinned_uniforms(SN, 0x5EED))
    a, b = E.bounds(RAGGED)[4]
    assert np.isnan(dense[a:b]).all() and np.isnan(dec[a:b]).all() and not np.isnan(dec[:a]).all()


# ------------------------------------------------------------------ D. ranges
@pytest.mark.parametrize("which", ["flat", "ragged"])
def test_qsgd_quantize_ranges_at_the_guard(which):
    """choco_qsgd_quantize_range over [0, 8192) and [8192, SN): each range message is the
    oracle's pack of the slices (its padding included)."""
    from chocosgd_amd import codec
    if which == "flat":
        q, lens, norms = 4, [SN], np.array([1.0], dtype=F32)
        x, xhat = guard_input("1", q, False)
    else:
        q, lens, norms = 16, RAGGED, RAGGED_NORMS["near"]
        x, xhat = ragged_input(q, True)
    seed, offset = 0x77AA, 5
    d = E.delta_of(x, xhat)
    lvl, _, _, _ = oracle_message(d, lens, norms, q, False, device_uniforms(SN, seed, offset))
    xd, hd, nd, so = dev(x), dev(xhat), dev(norms), seg_table(lens)
    for e0, e1 in ((0, 8192), (8192, SN)):
        part = torch.full((codec.qsgd_packed_bytes(e1 - e0, q),), 0xFF, dtype=torch.uint8, device=DEV)
        codec.qsgd_quantize_range(xd, q, nd, e0, e1, part, xhat=hd, seg_off=so, nseg=len(lens), seed=seed,
                                  offset=offset)
        assert np.array_equal(host(part), O.qsgd_pack(lvl[e0:e1], d[e0:e1], q)), (e0, e1)


# ------------------------------------------------------------------ E. device norms
SCALES = {"2^-140": 2.0 ** -140, "2^-45": 2.0 ** -45, "1": 1.0, "2^100": 2.0 ** 100, "2^120": 2.0 ** 120}
NORM_CASES = [("flat", (c,), None) for c in SCALES]
NORM_CASES += [("ragged", tuple(list(SCALES)[(i + r) % 5] for i in range(5)), None) for r in (0, 2)]
NORM_CASES += [(lay, ("1",) * len(E.QLAYOUTS[lay]), sp) for lay in ("flat", "ragged") for sp in ("zero", "inf", "nan")]
SPECIAL_SEG = {"zero": 2, "inf": 1, "nan": 3}  # the tensor of `ragged` that takes it


@functools.lru_cache(maxsize=None)
def scaled_case(layout, scales, special):
    """(x, xhat, mem) of randn * c per tensor (x_hat and memory at the same scale); `special`:
    one tensor all zero (x == x_hat, memory too), or holding one inf or one NaN in x."""
    lens = E.QLAYOUTS[layout]
    rng = np.random.default_rng([len(lens), sum(ord(ch) for ch in "".join(scales)), len(special or "")])
    c = np.concatenate([np.full(m, SCALES[k]) for m, k in zip(lens, scales)])
    x, xhat, mem = ((rng.standard_normal(SN) * c * f).astype(F32) for f in (1.0, 0.5, 1.0))
    if special:
        a, b = E.bounds(lens)[SPECIAL_SEG[special] if len(lens) > 1 else 0]
        if special == "zero":
            x[a:b] = xhat[a:b]
            mem[a:b] = xhat[a:b]
        else:
            x[a + (b - a) // 3] = np.inf if special == "inf" else np.nan
    return tuple(E.frozen(v) for v in (x, xhat, mem))


def run_device_norms(layout, scales, special, mode, q=4, seed=0xD00D, offset=9):
    """One qsgd_compress with device norms; returns (got norms, oracle norms)."""
    from chocosgd_amd import codec
    lens = E.QLAYOUTS[layout]
    x, xhat, mem = scaled_case(layout, scales, special)
    if mode == "plain":
        if special == "zero":  # (without x_hat the zero tensor is zero in x itself)
            x = x.copy()
            a, b = E.bounds(lens)[SPECIAL_SEG[special] if len(lens) > 1 else 0]
            x[a:b] = 0
        xhat = None
    xd = dev(x)
    packed, norms, dense = codec.qsgd_compress(xd, q, xhat=dev(xhat), seg_off=seg_table(lens), nseg=len(lens),
                                               seed=seed, offset=offset, want_dense=True,
                                               gossip=(dev(mem), GAMMA) if mode == "gossip" else None)
    with np.errstate(all="ignore"):
        if mode == "gossip":
            x = O.gossip_step(x, mem, xhat, GAMMA)
            assert same_bits(host(xd), x)
        d = E.delta_of(x, xhat)
        want = O.l2_norms(d, lens)
    got = host(norms)
    print(f"{layout} {scales} {special} {mode}: norms {got} oracle {want}")
    ok = E.within_one_ulp(got, want)
    assert ok.all(), f"norms {got} against {want}"
    # levels, wire and dense: bit-exact, the oracle fed the device's norms
    check_message(packed, norms, dense, d, lens, got, q, False, device_uniforms(SN, seed, offset))
    return got, want


@pytest.mark.parametrize("mode", ["plain", "xhat", "gossip"])
@pytest.mark.parametrize("layout,scales,special", NORM_CASES,
                         ids=[f"{lay}-{'/'.join(sc)}" + (f"-{sp}" if sp else "") for lay, sc, sp in NORM_CASES])
def test_qsgd_device_norms_at_extreme_scales(layout, scales, special, mode):
    """Subnormal inputs (2^-140) up to norms next to FLT_MAX (2^120), every tensor of
    `ragged` at another scale; an all-zero tensor (norm 0, NaN dense), one inf, one NaN."""
    got, want = run_device_norms(layout, scales, special, mode)
    if special:
        i = SPECIAL_SEG[special] if layout == "ragged" else 0
        assert {"zero": got[i] == 0, "inf": np.isposinf(got[i]), "nan": np.isnan(got[i])}[special]
        assert np.isfinite(np.delete(got, i)).all() and (np.delete(got, i) > 0).all()
    else:
        assert np.isfinite(got).all() and (got > 0).all()
    if "2^-140" in scales:
        assert (got[[k == "2^-140" for k in scales]] < np.finfo(F32).tiny).all()  # a subnormal norm


@pytest.mark.parametrize("mode", ["plain", "xhat", "gossip"])
@pytest.mark.parametrize("layout", ["flat", "ragged"])
def test_qsgd_norm_accumulators_reset_after_nonfinite(layout, mode):
    """The fp64 accumulators reset themselves through an atomic exchange: directly after a call
    that summed inf, and after one that summed NaN, the ordinary case's norms are the
    oracle's again (same device, same stream, same workspace)."""
    ones = ("1",) * len(E.QLAYOUTS[layout])
    for special in ("inf", "nan"):
        got, _ = run_device_norms(layout, ones, special, mode)
        assert not np.isfinite(got).all()
        got, _ = run_device_norms(layout, ones, None, mode)
        assert np.isfinite(got).all() and (got > 0).all(), special


# ------------------------------------------------------------------ F. sign pack
@functools.lru_cache(maxsize=None)
def sign_case(layout, nonfinite):
    return tuple(E.frozen(v) if isinstance(v, np.ndarray) else v
                 for v in E.sign_specials(E.SIGN_N, E.SIGN_LAYOUTS[layout], nonfinite=nonfinite))


def run_sign(layout, nonfinite, mode, entry):
    """One sign message through `entry` ("whole": sign_compress; "ranges": three
    sign_compress_range calls, twice over); words, norms, unpack and x_new against the oracle."""
    from chocosgd_amd import codec
    lens = E.SIGN_LAYOUTS[layout]
    n, nseg, so = E.SIGN_N, len(lens), seg_table(lens)
    d_plain, x, xhat, mem, kinds = sign_case(layout, nonfinite)
    if mode == "plain":
        x, xhat = d_plain, None
    with np.errstate(all="ignore"):
        x_new = O.gossip_step(x, mem, xhat, GAMMA) if mode == "gossip" else x
        d = E.delta_of(x_new, xhat)
        want_words, want_norms = O.sign_pack(d), O.l1_norms(d, lens)
    hd, md = dev(xhat), dev(mem)
    for rep in range(1 if entry == "whole" else 2):
        xd = dev(x)
        g = (md, GAMMA) if mode == "gossip" else None
        if entry == "whole":
            packed, norms = codec.sign_compress(xd, xhat=hd, seg_off=so, nseg=nseg, gossip=g)
        else:
            packed = torch.full((codec.sign_words(n),), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
            norms = torch.full((nseg,), -1.0, device=DEV)
            ranges = codec.sign_chunks(n, 3)
            assert len(ranges) == 3 and ranges[0][0] == 0 and ranges[-1][1] == codec.sign_words(n)
            for i, (w0, w1) in enumerate(ranges):
                codec.sign_compress_range(xd, w0, w1, i == len(ranges) - 1, xhat=hd, seg_off=so, nseg=nseg, gossip=g,
                                          out=(packed, norms))
        got_words, got = host(packed), host(norms)
        bad = np.nonzero(got_words != want_words)[0]
        assert bad.size == 0, f"rep {rep}: {bad.size} words differ, first at {bad[:8]}"
        print(f"{layout} {mode} {entry} rep {rep}: norms {got} oracle {want_norms}")
        assert E.within_one_ulp(got, want_norms).all(), f"rep {rep}: norms {got} against {want_norms}"
        if mode == "gossip":
            assert same_bits(host(xd), x_new), rep
        assert same_bits(host(codec.sign_unpack(packed, n)), O.sign_unpack(want_words, n)), rep
    return got


@pytest.mark.parametrize("entry", ["whole", "ranges"])
@pytest.mark.parametrize("mode", ["plain", "xhat", "gossip"])
@pytest.mark.parametrize("layout", list(E.SIGN_LAYOUTS))
def test_sign_pack_special_values(layout, mode, entry):
    """d < 0 sets the bit; +-0, NaN and the padding encode as "+"; -1e-45 is negative.  NaN,
    +-inf, +-0, +-1e-45 and x == x_hat at every tensor's ends, on both sides of every row
    boundary of the (32, N') view and next to the padded columns.  The inf and NaN tensors'
    norms match as classes, the zero tensor's is exactly 0, and the ordinary message packed
    directly afterwards has clean norms."""
    got = run_sign(layout, True, mode, entry)
    if layout == "ragged":
        assert got[E.SIGN_ZERO_SEG] == 0 and np.isnan(got[E.SIGN_NAN_SEG]) and np.isposinf(got[E.SIGN_INF_SEG])
        assert np.isfinite(got[[0, 2]]).all() and (got[[0, 2]] >= 0).all()
    else:
        assert np.isnan(got[0])
    got = run_sign(layout, False, mode, entry)
    assert np.isfinite(got).all()
    if layout == "ragged":
        assert got[E.SIGN_ZERO_SEG] == 0
