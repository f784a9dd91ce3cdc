"""The model of the top-k warm-start controller (tests/_topk_controller.py) held to its own
claims, so that it is not just a copy of the code's mistakes: each piece is checked against
an independent statement of its contract.  No GPU."""
import math
import random

import numpy as np
import pytest

import _topk_controller as M

I32_MIN = 0x80000000


# ------------------------------------------------------------------------------ drift
def _i32(b):
    return b - (1 << 32) if b >= 1 << 31 else b


def _drift_contract(T, t_prev, d_prev_bits, valid):
    """0 unless the last two moves share a sign; else the move of smaller magnitude; +-2^30."""
    if not valid or t_prev == 0:
        return 0
    a, b = T - t_prev, _i32(d_prev_bits)
    if a * b <= 0:
        return 0
    v = a if abs(a) <= abs(b) else b
    return max(-(1 << 30), min(1 << 30, v))


def _triples():
    rnd = random.Random(1)
    edge = [0, 1, 2, 0x3F800000, 0x7F7FFFFF, 0x7F800000, 0x7FFFFFFF]
    dbits = [0, 1, 0xFFFFFFFF, I32_MIN, I32_MIN + 1, 0x7FFFFFFF, 1 << 30, (1 << 30) + 1, (-(1 << 30)) & M.U32,
             (-(1 << 30) - 1) & M.U32]
    out = [(T, t, d) for T in edge for t in edge for d in dbits]
    for _ in range(4000):
        t = rnd.randrange(0, 1 << 31)
        span = rnd.choice([4, 1 << 10, 1 << 20, 1 << 31])
        T = min(max(t + rnd.randrange(-span, span + 1), 0), (1 << 31) - 1)
        d = rnd.randrange(-span, span + 1) & M.U32
        out.append((T, t, d))
    return out


def test_window_drift_contract():
    n_nonzero = 0
    for T, t, d in _triples():
        for valid in (True, False):
            got = M.window_drift(T, t, d, valid)
            assert got == _drift_contract(T, t, d, valid), (T, t, d, valid)
            assert -(1 << 30) <= got <= 1 << 30
            n_nonzero += got != 0
    assert n_nonzero > 500   # the triples reach the non-trivial branch
    # the named edges
    assert M.window_drift(100, 0, 5, True) == 0            # t_prev = 0: no previous key
    assert M.window_drift(100, 100, 5, True) == 0          # a move of 0
    assert M.window_drift(105, 100, 0, True) == 0
    assert M.window_drift(105, 100, I32_MIN, True) == 0    # INT32_MIN bits: a negative move
    assert M.window_drift(1, (1 << 31) - 1, I32_MIN, True) == -(1 << 30)
    assert M.window_drift(105, 100, 3, True) == 3 and M.window_drift(103, 100, 5, True) == 3
    assert M.window_drift(95, 100, (-3) & M.U32, True) == -3 and M.window_drift(97, 100, (-5) & M.U32, True) == -3


def test_drift_trusted_contract():
    hits = 0
    for T, t, d in _triples():
        for valid in (True, False):
            want = valid and t != 0 and abs(T - t - _i32(d)) < abs(T - t)
            assert M.drift_trusted(T, t, d, valid) == want, (T, t, d, valid)
            hits += want
    assert hits > 300


def test_nk_tag_is_32_bit_and_tells_shapes_apart():
    shapes = [(M.N_FIRST, 655), (M.N_FIRST, 6553), (M.N_MAIN, 2621), (M.N_MAIN, 26214), (M.N_LARGE, 10485),
              (2 ** 31 - 2, 2 ** 31 - 3), (2 ** 31 - 2, 1)]
    tags = [M.nk_tag(n, k) for n, k in shapes]
    assert all(0 < t <= M.U32 for t in tags) and len(set(tags)) == len(tags)
    assert M.nk_tag(100003, 1000) == ((100003 * 2654435761) % 2 ** 32) ^ (1000 * 40503) ^ 1


# ------------------------------------------------------------------------------ next_window
N, SEED = M.N_MAIN, 4242


def _skeys(seed, scale=1.0):
    return M.sorted_keys(M.normal(N, seed) * np.float32(scale))


def _sample_like_window(skeys, k):
    """A cold window as the sample makes one: edges at the count levels k (1 +- 1/2), no margin."""
    lo, hi = M.kth_key(skeys, k + k // 2), M.kth_key(skeys, k - k // 2) + 1
    sh, w_hi = M._fit(lo, hi)
    return (lo, w_hi, sh, 0)


def _chain(k, seeds, scale=lambda c: 1.0):
    """next_window call after call: every call uses the window the previous one prepared."""
    win, out = None, []
    for c, seed in enumerate(seeds):
        sk = _skeys(seed, scale(c))
        if win is None:
            win = _sample_like_window(sk, k)
        fb, G, jstar = M.predict_fallback(sk, k, win, 0)
        T = M.kth_key(sk, k)
        nxt, br = (M.next_window(G, win, T, N, k, 0) if not fb else (None, None))
        out.append({"sk": sk, "used": win, "fallback": fb, "G": G, "jstar": jstar, "T": T, "next": nxt, "br": br})
        if fb:
            break
        win = nxt
    return out


@pytest.fixture(scope="module", params=[0.99, 0.9], ids=["k1pct", "k10pct"])
def iid(request):
    """30 independent redraws at n = 262,147, computed once."""
    k = M.topk_k(N, request.param)
    return k, _chain(k, range(SEED, SEED + 30))


def test_next_window_holds_the_kth_key(iid):
    k, chain = iid
    for r in chain:
        s_lo, s_hi, shift, m = r["next"]
        assert s_lo <= r["T"] < s_hi
        # ... and aims where it says: at least k (1 + m) keys above the floor, at most k (1 - m)
        # above the ceiling (edges inside the window the call used)
        if "extended_down" not in r["br"]:
            assert M.count_ge(r["sk"], s_lo) >= k + k * m // 1024
        if "extended_up" not in r["br"]:
            assert M.count_ge(r["sk"], s_hi) <= k - k * m // 1024 or s_hi >= r["used"][1]


def test_next_window_width_is_255_buckets_of_the_smallest_shift(iid):
    k, chain = iid
    for r in chain:
        s_lo, s_hi, shift, m = r["next"]
        assert s_hi - s_lo == 255 << shift
        # the span it has to cover, restated from the counts: from the floor to the first bucket
        # edge of the used window with at most k (1 - m) keys above it
        u_lo, u_hi, u_sh, _ = r["used"]
        hi_t = k - k * m // 1024
        edges = [u_lo + (j << u_sh) for j in range(255)] + [u_hi]
        x_hi = next((e for e in edges if M.count_ge(r["sk"], e) <= hi_t), None)
        if x_hi is not None:
            span = x_hi - s_lo
            assert (255 << shift) >= span and (shift == 0 or (255 << (shift - 1)) < span)


def test_margin_stays_at_its_floor_on_iid_redraws(iid):
    """The round-4 regression as a property: counting the outward rounding of the edges (or the
    draw-to-draw count noise) as drift doubled m call after call."""
    k, chain = iid
    assert len(chain) == 30 and not any(r["fallback"] for r in chain)
    assert [r["next"][3] for r in chain] == [M.warm_m0(k)] * 30


def test_margin_floor_follows_the_count_noise():
    """warm_m0: kWarmM0 where 8 sqrt(2 / k) of k is less (the bench's sizes, untouched), that
    noise bound below; never above kWarmMMax."""
    assert M.warm_m0(1_000_000) == M.warm_m0(335_545) == M.K_WARM_M0
    assert M.warm_m0(250_000) == 24
    for k in [1, 2, 100, 655, 2621, 6553, 10485, 26214, 104858, 335_544]:
        m = M.warm_m0(k)
        assert M.K_WARM_M0 <= m <= M.K_WARM_M_MAX
        assert m == M.K_WARM_M_MAX or (m - 1) / 1024.0 < 8.0 * math.sqrt(2.0 / k) <= m / 1024.0


@pytest.mark.parametrize("ratio", [0.99, 0.9])
@pytest.mark.parametrize("rate", [0.9, 0.97, 1.0 / 0.97, 1.0 / 0.9])
def test_margin_never_exceeds_its_cap(ratio, rate):
    k = M.topk_k(N, ratio)
    chain = _chain(k, range(SEED, SEED + 12), scale=lambda c: rate ** c)
    assert len(chain) >= 2
    for r in chain:
        if not r["fallback"]:
            assert M.warm_m0(k) <= r["next"][3] <= M.K_WARM_M_MAX


def test_kth_bucket_fits_the_select(iid):
    """The bucket of the k-th key in a floor-margin window holds at most kMCap keys: the GPU
    file's inputs do not fall back on their own account."""
    k, chain = iid
    for r in chain[1:]:
        assert r["used"][3] == M.warm_m0(k)
        assert r["G"][r["jstar"]] - r["G"][r["jstar"] + 1] <= M.K_MCAP


def test_fallback_window_holds_the_kth_key_and_is_bin_rounded():
    for ratio in (0.99, 0.9, 0.5):
        k = M.topk_k(N, ratio)
        sk = _skeys(SEED)
        s_lo, s_hi, shift, m = M.fallback_window(sk, N, k)
        assert m == 0 and s_lo % (1 << 20) == 0 and s_hi - s_lo == 255 << shift
        assert s_lo <= M.kth_key(sk, k) < s_hi
        assert M.count_ge(sk, s_lo) >= k + k // 8 and M.count_ge(sk, s_hi) < max(1, k - k // 8)


# ------------------------------------------------------------------------------ predict_fallback
def test_predict_fallback_reasons():
    k = M.topk_k(N, 0.99)
    sk = _skeys(SEED)
    T = M.kth_key(sk, k)
    good = _sample_like_window(sk, k)
    fb, G, jstar = M.predict_fallback(sk, k, good, 0)
    assert not fb and G == sorted(G, reverse=True) and len(G) == 256
    assert good[0] + (jstar << good[2]) <= T < good[0] + ((jstar + 1) << good[2])
    assert M.predict_fallback(sk, k, good, 1)[0] and M.predict_fallback(sk, k, good, 2)[0]   # overflow word
    assert M.predict_fallback(sk, k, (T + 1, T + 256, 0, 0), 0)[0]                          # too few candidates
    assert M.predict_fallback(sk, k, (T - 255, T, 0, 0), 0)[0]                              # T is "sure"
    tie = np.sort(np.concatenate([sk[:N - k - 20000], np.full(k + 20000, T, dtype=np.int64)]))
    fb, G, jstar = M.predict_fallback(tie, k, good, 0)                                       # bucket j* too large
    assert fb and jstar is not None and G[jstar] - G[jstar + 1] > M.K_MCAP


# ------------------------------------------------------------------------------ step
NK = (N, 2621)
TAG = M.nk_tag(*NK)


def _st(**kw):
    s = M.fresh_state()
    s.update(kw)
    return s


def test_step_warm_hit():
    s = _st(t_prev=1000, d_prev=10, sh_lo=900, sh_hi=1200, sh_nk=TAG, sh_hits=1, d_cand=10, d_trust=1, backoff=256)
    nxt, ev, ch = M.step(s, (900, 1200, 1, 227), 1012, False, *NK, prepared=(950, 1205))
    assert (ev, ch) == ("warm_hit", "halved")
    assert nxt == _st(t_prev=1012, d_prev=12, sh_lo=950, sh_hi=1205, sh_nk=TAG, sh_hits=0, d_cand=10, d_trust=2,
                      backoff=128, cold_left=0)
    assert M.step(_st(backoff=64), (900, 1200, 1, 20), 1012, False, *NK, prepared=(1, 2))[0]["backoff"] == 64
    assert M.step(_st(), (900, 1200, 1, 20), 1012, False, *NK, prepared=(1, 2))[0]["backoff"] == 64


def test_step_warm_miss_and_the_three_resets():
    s = _st(t_prev=1000, d_prev=10, sh_lo=900, sh_hi=1200, sh_nk=TAG, sh_hits=1, d_cand=10, d_trust=3, backoff=64)
    nxt, ev, ch = M.step(s, (900, 1200, 1, 227), 0, True, *NK)
    assert (ev, ch) == ("warm_miss", "doubled")
    # reset after a fallback: the drift words, the shadow's tag (so the shadow cannot hit) and
    # the hit streak; the stale shadow edges stay
    assert nxt == _st(sh_lo=900, sh_hi=1200, backoff=128, cold_left=128)
    assert M.step(_st(), (900, 1200, 1, 227), 0, True, *NK)[0]["cold_left"] == 64           # the first run
    assert M.step(_st(backoff=4096), (900, 1200, 1, 227), 0, True, *NK)[0]["backoff"] == 4096
    # ... on a cold call's fallback too (no cold run started)
    nxt, ev, ch = M.step(s, (900, 1200, 1, 0), 0, True, *NK)
    assert ev == "cold_call" and nxt == _st(sh_lo=900, sh_hi=1200, sh_hits=1, backoff=64)
    # ... and on a cold-run step's fallback
    nxt, ev, ch = M.step(dict(s, cold_left=5), (900, 1200, 1, 0), 0, True, *NK)
    assert ev == "cold_run_step" and nxt == _st(sh_lo=900, sh_hi=1200, backoff=64, cold_left=4)


def test_step_cold_run_step_and_shadow_exit():
    s = _st(t_prev=1000, sh_lo=900, sh_hi=1200, sh_nk=TAG, backoff=64, cold_left=60)
    nxt, ev, _ = M.step(s, (800, 1400, 2, 0), 1100, False, *NK, prepared=(950, 1300))
    assert ev == "cold_run_step" and (nxt["cold_left"], nxt["sh_hits"]) == (59, 1)
    nxt2, ev, _ = M.step(nxt, (800, 1400, 2, 0), 1299, False, *NK, prepared=(1000, 1400))
    assert ev == "shadow_exit" and (nxt2["cold_left"], nxt2["sh_hits"], nxt2["backoff"]) == (0, 0, 64)
    # the shadow's ceiling is exclusive, another shape's shadow never hits, a miss ends the streak
    assert M.step(nxt, (800, 1400, 2, 0), 1300, False, *NK, prepared=(1, 2))[0]["sh_hits"] == 0
    assert M.step(dict(nxt, sh_nk=TAG ^ 2), (800, 1400, 2, 0), 1100, False, *NK, prepared=(1, 2))[0]["sh_hits"] == 0
    # counting down to the end
    nxt3, ev, _ = M.step(dict(s, cold_left=1, sh_nk=0), (800, 1400, 2, 0), 1100, False, *NK, prepared=(1, 2))
    assert ev == "cold_run_step" and nxt3["cold_left"] == 0


def test_step_cold_call_and_shape_change():
    nxt, ev, ch = M.step(_st(), (800, 1400, 2, 0), 1100, False, *NK, prepared=(950, 1300))
    assert (ev, ch) == ("cold_call", None)
    assert nxt == _st(t_prev=1100, sh_lo=950, sh_hi=1300, sh_nk=TAG)
    other = M.step(nxt, (5, 600, 2, 0), 300, False, M.N_FIRST, 655, prepared=(200, 400))[0]
    assert other["d_prev"] == 0 and other["d_cand"] == 0 and other["sh_nk"] == M.nk_tag(M.N_FIRST, 655)


# ------------------------------------------------------------------------------ host side
def test_expect_sample():
    n, k = NK
    assert M.expect_sample(None, n, k, 0, False, True) == "k1"            # first call on the workspace
    assert M.expect_sample((n, k + 1), n, k, 0, False, True) == "k1"      # another shape
    assert M.expect_sample((n, k), n, k, 0, False, False) == "k1"         # warm start off
    assert M.expect_sample((n, k), n, k, 0, False, True) is None
    assert M.expect_sample((n, k), n, k, 3, False, True) == "k2"          # cold run: K2's prologue
    assert M.expect_sample((n, k), n, k, 3, True, True) == "k1"           # ... never with the fused step
    assert M.expect_sample((n, k), n, k, 0, True, True) is None
    stale = (1, 2, 3, 20, n, k + 1, 1)
    assert M.expect_sample((n, k), n, k, 0, False, True, stale) == "k2"
    assert M.expect_sample((n, k), n, k, 0, True, True, stale) is None


# ------------------------------------------------------------------------------ predictability
def test_gpu_inputs_are_predictable():
    """The inputs of tests/test_gpu_topk_controller.py, from the same generators: no NaN / inf,
    and outside the tie sequence fewer than kMCap keys equal the k-th -- so the model predicts
    every fallback from the keys and the window alone and the GPU file may demand equality."""
    cases = M.gpu_cases()
    assert len(cases) >= 20
    for name, make in cases.items():
        for call in make():
            d, k = call["d"], call["k"]
            assert d.dtype == np.float32 and d.size == call["n"] > M.K_SMALL_N and 0 < k < d.size, name
            assert np.isfinite(d).all(), name
            keys = M.keys(d)
            T = np.partition(keys, d.size - k)[d.size - k]
            ties = int(np.count_nonzero(keys == T))
            assert (ties > M.K_MCAP) if call["tie"] else (ties < 64), (name, ties)
