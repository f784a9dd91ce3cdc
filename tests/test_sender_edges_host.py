"""Conditions on the sender edge inputs (tests/_sender_edges.py) and on the oracle they are
checked against: they keep tests/test_gpu_senders.py from silently losing the coverage it is
written for.  No GPU.

  * every in-range pinned norm and every q in 1..16: enough 512-element slabs of the full tiles
    with both flagged and unflagged groups, with none and with only flagged ones; enough
    elements below the low threshold and above the high one; values within 3 ulps on both
    sides of each threshold (measured on t = RN(s |d|) and on q0 = RN(t RN(1/N)));
  * the oracle's own division on every ladder pair equals the exactly rounded quotient
    (fractions.Fraction, round to nearest even, subnormals included): a numpy build that
    flushed denormals would not pass;
  * O.qsgd_pack clamps levels >= s to s and sends NaN levels to 0.
"""
from fractions import Fraction

import numpy as np
import pytest

import _sender_edges as E
from conftest import same_bits
from oracle import choco_oracle as O

F32 = np.float32
IN_RANGE = {"2^-30": F32(2.0 ** -30), "2^96": F32(2.0 ** 96), "1": F32(1.0),
            "0x1.fffffep+0": E.prev32(F32(2.0)), "3e-5": F32(3e-5)}
OUT_OF_RANGE = {"prev(2^-30)": E.prev32(F32(2.0 ** -30)), "next(2^96)": E.next32(F32(2.0 ** 96)),
                "2^-126": F32(2.0 ** -126), "2^-140": F32(2.0 ** -140), "FLT_MAX": np.finfo(F32).max}
ALL_Q = list(range(1, 17))


def coverage(d, N, s):
    """Class counts over the full tiles: (low, high, mixed, none, all)."""
    low, high = E.classify(d[:3 * E.TILE], N, s)
    return (int(low.sum()), int(high.sum())) + E.slab_classes(d, N, s)


def near_thresholds(d, N, s):
    """(below, above) x (low threshold, high threshold): counts of full-tile elements within 3
    ulps of each threshold, on each side."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        t = (F32(s) * np.abs(d[:3 * E.TILE])).astype(F32)
        q0 = (t * (F32(1.0) / N)).astype(F32)
        tlo = N * E.T_LO_FACTOR
    fin = np.isfinite(t) & (t != 0)
    dt = E.ordered(t) - E.ordered(tlo)
    fq = np.isfinite(q0)
    dq = E.ordered(q0) - E.ordered(F32(128.0))
    return (int((fin & (dt < 0) & (dt >= -3)).sum()), int((fin & (dt >= 0) & (dt <= 3)).sum()),
            int((fq & (dq <= 0) & (dq >= -3)).sum()), int((fq & (dq > 0) & (dq <= 3)).sum()))


@pytest.mark.parametrize("q", ALL_Q)
@pytest.mark.parametrize("name", list(IN_RANGE))
def test_pinned_delta_covers_the_guard(name, q):
    N, s = IN_RANGE[name], 2 ** q - 1
    d, is_ladder = E.pinned_delta(N, s)
    x, xhat = E.under_xhat(d, is_ladder)
    for what, dd in (("plain", d), ("xhat", E.delta_of(x, xhat))):
        low, high, mixed, none, full = coverage(dd, N, s)
        print(f"N={name} q={q} {what}: low {low} high {high} slabs mixed {mixed} none {none} all {full}")
        assert mixed >= 8 and none >= 4 and full >= 4, (what, mixed, none, full)
        assert low >= 100 and high >= 100, (what, low, high)
        lo_below, lo_above, hi_below, hi_above = near_thresholds(dd, N, s)
        assert min(lo_below, lo_above, hi_below, hi_above) >= 1, (what, lo_below, lo_above, hi_below, hi_above)
    # the second half of tile 1 is filler only and unflagged; the first half holds a flagged
    # element in every group; the partial tile holds specials
    assert not E.group_flags(d[E.TILE + 4096:2 * E.TILE], N, s).any()
    assert E.group_flags(d[E.TILE:E.TILE + 4096], N, s).all()
    tail = d[3 * E.TILE:]
    assert np.isnan(tail).any() and np.isinf(tail).any() and (tail == 0).any() and (np.abs(tail) == N).any()


def test_under_xhat_is_exact_on_the_ladder():
    for N in list(IN_RANGE.values()) + list(OUT_OF_RANGE.values()) + [F32(0), F32(np.inf), F32(np.nan)]:
        for q in (1, 4, 16):
            d, is_ladder = E.pinned_delta(N, 2 ** q - 1)
            x, xhat = E.under_xhat(d, is_ladder)
            got = E.delta_of(x, xhat)
            assert same_bits(got[is_ladder], d[is_ladder])
            neg0 = is_ladder & (d == 0) & np.signbit(d)
            assert neg0.any() and np.signbit(got[neg0]).all()


@pytest.mark.parametrize("q", [4, 16])
def test_ragged_delta_covers_every_tensor(q):
    """Each in-range tensor of `ragged` holds low, high, flagged and unflagged groups and
    values next to both thresholds; the full tiles' boundaries are the documented ones."""
    s = 2 ** q - 1
    norms = np.array([1.0, E.prev32(F32(2.0 ** -30)), 2.0 ** 96, 3e-5, 0.0], dtype=F32)
    d, is_ladder = E.ragged_delta(norms, s)
    segs = E.bounds(E.QLAYOUTS["ragged"])
    assert [a for a, _ in segs] == [0, 5000, 8195, 16385, 24576]
    for i in (0, 2, 3):
        a, b = segs[i]
        a8, b8 = -(-a // 8) * 8, b // 8 * 8
        dd = d[a8:b8]
        low, high = E.classify(dd, norms[i], s)
        flags = E.group_flags(dd, norms[i], s)
        print(f"tensor {i} q={q}: low {low.sum()} high {high.sum()} flagged groups {flags.sum()} of {flags.size}")
        assert low.sum() >= 50 and high.sum() >= 30 and flags.any() and not flags.all()
    for i, (a, b) in enumerate(segs):
        assert np.isnan(d[a:b]).any() and np.isinf(d[a:b]).any() and (d[a:b] == 0).any()
    x, xhat = E.under_xhat(d, is_ladder)
    assert same_bits(E.delta_of(x, xhat)[is_ladder], d[is_ladder])


@pytest.mark.parametrize("q", [1, 4, 8, 16])
@pytest.mark.parametrize("name", list(IN_RANGE))
def test_sharp_uniforms_show_the_last_bit(name, q):
    """Under the sharp uniforms the oracle's level is the floor at the elements given the
    fraction itself and the floor + 1 at those given the value below it; moving the quotient
    by one ulp (here: the fraction) flips at least 9 in 10 of each kind in the full tiles."""
    N, s = IN_RANGE[name], 2 ** q - 1
    d, _ = E.pinned_delta(N, s)
    u = E.sharp_uniforms(d, [E.SN], [N], s, 0x5EED)
    with np.errstate(all="ignore"):
        lf = ((F32(s) * np.abs(d)).astype(F32) / N).astype(F32)
        pl = np.floor(lf)
        frac = (lf - pl).astype(F32)
        lvl = O.qsgd_levels(d, s, u, N)
    full = np.arange(E.SN) < 3 * E.TILE
    stay, step = full & (u == frac) & (frac > 0), full & (u < frac) & (E.ordered(frac) - E.ordered(u) == 1)
    print(f"N={name} q={q}: {stay.sum()} elements at the fraction, {step.sum()} one below it")
    assert stay.sum() >= 5000 and step.sum() >= 5000
    assert (lvl[stay] == pl[stay]).all() and (lvl[step] == pl[step] + 1).all()
    with np.errstate(all="ignore"):
        ulp = np.abs(np.spacing(lf))  # one ulp of the quotient, as a change of its fraction
    assert ((frac + ulp)[stay] > u[stay]).all()             # an ulp up: these would step
    assert ((frac - ulp)[step] <= u[step]).mean() >= 0.9     # an ulp down: these would stay


# ------------------------------------------------------------------------------ the oracle
def rn32(fr):
    """The fp32 value nearest the non-negative Fraction fr (ties to even, subnormals, inf)."""
    if fr == 0:
        return F32(0)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    e = max(e, -126)
    quantum = Fraction(2) ** (e - 23)
    n = fr / quantum
    k = n.numerator // n.denominator
    rem = n - k
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and k % 2 == 1):
        k += 1
    val = k * quantum
    if val >= Fraction(2) ** 128:
        return F32(np.inf)
    return F32(float(val))


def olevels(d, s, u, N):
    with np.errstate(over="ignore"):
        return O.qsgd_levels(d, s, u, N)


def test_rn32_itself():
    assert rn32(Fraction(1, 3)) == F32(1 / 3) and rn32(Fraction(2) ** -149) == F32(1e-45)
    assert rn32(Fraction(2) ** -150) == 0 and rn32(Fraction(3, 2) * Fraction(2) ** -149) == F32(2.8e-45)
    assert rn32(Fraction(2) ** 128 - Fraction(2) ** 103) == np.inf
    assert rn32(Fraction(2) ** 128 - Fraction(2) ** 103 - 1) == np.finfo(F32).max
    assert rn32(Fraction(16777217)) == F32(16777216) and rn32(Fraction(16777219)) == F32(16777220)


@pytest.mark.parametrize("name", list(IN_RANGE) + list(OUT_OF_RANGE))
def test_oracle_division_is_exactly_rounded(name):
    """O.qsgd_levels' level_float on every ladder pair against exact rationals: with u = 2
    the level is floor(lf); with u = lf - floor(lf) it stays, with the fp32 value below
    that it steps up -- together they pin lf to the exactly rounded RN(RN(s |d|) / N)."""
    N = {**IN_RANGE, **OUT_OF_RANGE}[name]
    Nf = Fraction(float(N))
    pairs = fractional = 0
    for q in ALL_Q:
        s = 2 ** q - 1
        lad = np.unique(np.abs(E.ladder(N, s)))
        lad = lad[np.isfinite(lad)]
        t = np.array([rn32(s * Fraction(float(v))) for v in lad], dtype=F32)
        with np.errstate(over="ignore"):
            assert same_bits(t, (F32(s) * lad).astype(F32))
        lf = np.array([rn32(Fraction(float(v)) / Nf) if np.isfinite(v) else F32(np.inf) for v in t], dtype=F32)
        fin = np.isfinite(lf)
        assert fin.sum() >= 0.9 * lad.size
        pl = np.floor(lf)
        with np.errstate(invalid="ignore"):
            frac = (lf - pl).astype(F32)  # exact in fp32
        assert same_bits(olevels(lad, s, np.full(lad.size, 2.0, dtype=F32), N), pl)
        assert same_bits(olevels(lad[fin], s, frac[fin], N), pl[fin])
        pos = fin & (frac > 0)
        below = np.array([E.prev32(v) for v in frac[pos]], dtype=F32)
        assert same_bits(olevels(lad[pos], s, below, N), pl[pos] + 1)
        assert (pl[fin] == lf[fin]).any() and pos.any()
        pairs += int(lad.size)
        fractional += int(pos.sum())
    assert fractional >= 500  # pairs whose quotient is no integer (the subnormal norm has few)
    print(f"N={name}: {pairs} ladder pairs")


@pytest.mark.parametrize("q", ALL_Q)
def test_oracle_pack_clamps(q):
    """Levels >= s are sent as s, NaN levels as 0; the sign plane is d < 0 (so -0 and NaN are +)."""
    s = 2 ** q - 1
    N = F32(3e-5)
    lad = E.ladder(N, s)
    lad = np.concatenate([lad, -lad]).astype(F32)
    lvl = olevels(lad, s, np.zeros(lad.size, dtype=F32), N)
    assert np.isnan(lvl).any() and (lvl > s).any() and (lvl == s).any() and (lvl == s + 1).any() and np.isinf(lvl).any()
    levels, neg = O.qsgd_unpack(O.qsgd_pack(lvl, lad, q), lad.size, q)
    want = np.where(np.isnan(lvl), 0, np.minimum(np.nan_to_num(lvl, nan=0.0, posinf=float(s)), s)).astype(np.uint64)
    assert np.array_equal(levels, want)
    assert levels[np.isnan(lvl)].max() == 0 and levels[~np.isnan(lvl) & (lvl >= s)].min() == s
    with np.errstate(invalid="ignore"):
        assert np.array_equal(neg, lad < 0)
    assert not neg[np.isnan(lad)].any() and not neg[lad == 0].any()


# ------------------------------------------------------------------------------ sign inputs
@pytest.mark.parametrize("layout", list(E.SIGN_LAYOUTS))
def test_sign_specials_cover_the_edges(layout):
    lens = E.SIGN_LAYOUTS[layout]
    n, Np = E.SIGN_N, O.sign_words(E.SIGN_N)
    assert Np == 2050 and sum(lens) == n
    d, x, xhat, mem, kinds = E.sign_specials(n, lens)
    assert set(kinds.values()) == set(E.FINITE_KINDS + E.NONFINITE_KINDS)
    pos = np.array(sorted(kinds))
    for a, b in E.bounds(lens):
        assert a in kinds and b - 1 in kinds
    for r in range(1, 32):
        assert r * Np - 1 in kinds and r * Np in kinds
    assert n - 1 in kinds and n - 31 * Np in kinds
    got = E.delta_of(x, xhat)
    assert same_bits(got[pos], d[pos])                         # exact at the special positions
    assert same_bits(mem[pos], xhat[pos])
    eq = np.array([p for p, k in kinds.items() if k == "equal"])
    assert (x[eq] == xhat[eq]).all() and (x[eq] != 0).all() and not np.signbit(got[eq]).any()
    l1 = O.l1_norms(got, lens)
    if layout == "ragged":
        a, b = E.bounds(lens)[E.SIGN_ZERO_SEG]
        assert (d[a:b] == 0).all() and np.signbit(d[a:b]).any() and not np.signbit(d[a:b]).all() and l1[3] == 0
        assert np.isnan(l1[E.SIGN_NAN_SEG]) and np.isinf(l1[E.SIGN_INF_SEG])
        assert np.isfinite(l1[[0, 2, 3]]).all()
    else:
        assert np.isnan(l1[0])
    dq, xq, xhq, _, kq = E.sign_specials(n, lens, nonfinite=False)
    assert np.isfinite(dq).all() and np.isfinite(xq).all() and set(kq.values()) == set(E.FINITE_KINDS)
    assert np.isfinite(O.l1_norms(E.delta_of(xq, xhq), lens)).all()
