"""A plain model of the flat top-k warm-start controller (chocosgd_amd/csrc/topk.hip,
`topk_finish_kernel` workgroup 0, and the host's choice in `launch_topk`).

Python ints and numpy float64 only: no torch, no GPU.  Each function restates one piece
of topk.hip or choco_common.h and names it.  tests/test_topk_controller_host.py holds this
model to its own contracts; tests/test_gpu_topk_controller.py holds the device to the model,
word by word, after every call.
"""
import math

import numpy as np

# topk.hip constants
K_NBUCKET = 256            # kNBucket
K_NMAYBE = 255             # kNMaybe
K_MCAP = 16384             # kMCap: max keys of bucket j* selected in LDS
K_SMALL_N = 65536          # kSmallN: at or below it one workgroup selects, no controller
K_COLD_MIN, K_COLD_MAX = 64, 4096   # kColdMin, kColdMax
K_SHADOW_EXIT = 2          # kShadowExit
K_WARM_M0 = 20             # kWarmM0
K_WARM_M_MAX = 512         # kWarmMMax
K_DRIFT_TRUST = 2          # kDriftTrust (choco_common.h)

U32 = 0xFFFFFFFF

STATE_WORDS = ("t_prev", "d_prev", "sh_lo", "sh_hi", "sh_nk", "sh_hits", "d_cand", "d_trust", "backoff",
               "cold_left")
EVENTS = ("warm_hit", "warm_miss", "cold_run_step", "shadow_exit", "cold_call")


def fresh_state():
    """A zero-filled workspace."""
    return {w: 0 for w in STATE_WORDS}


def _i32(bits):
    """(int32_t) of a uint32 word."""
    bits &= U32
    return bits - (1 << 32) if bits & 0x80000000 else bits


# ------------------------------------------------------------------------------ keys
def keys(d):
    """fkey of every element (choco_common.h `fkey`): the fp32 bits without the sign."""
    return np.ascontiguousarray(d, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def sorted_keys(d):
    """The keys in ascending order, int64 (what the counting functions below take)."""
    return np.sort(keys(d).astype(np.int64))


def kth_key(skeys, k):
    """T_exact: the k-th largest key (skeys ascending)."""
    return int(skeys[skeys.size - k])


def count_ge(skeys, t):
    """#{key >= t}."""
    return int(skeys.size - np.searchsorted(skeys, t, side="left"))


# ------------------------------------------------------------------------------ drift
def window_drift(T, t_prev, d_prev_bits, valid):
    """choco_common.h `window_drift`: the last move T - t_prev when it has the sign of the
    move before it (d_prev), clamped to the smaller of the two and to +-2^30."""
    if not valid or t_prev == 0:
        return 0
    dn = T - t_prev
    dp = _i32(d_prev_bits)
    if dp == 0 or dn == 0 or (dn > 0) != (dp > 0):
        return 0
    m = min(dn, dp) if dn > 0 else max(dn, dp)
    return max(-(1 << 30), min(1 << 30, m))


def drift_trusted(T, t_prev, cand_bits, valid):
    """choco_common.h `drift_trusted`: the proposed drift would have predicted T better than
    the previous key did."""
    if not valid or t_prev == 0 or (cand_bits & U32) == 0:
        return False
    e_static = T - t_prev
    e_drift = e_static - _i32(cand_bits)
    return abs(e_drift) < abs(e_static)


def nk_tag(n, k):
    """topk.hip `nk_tag`, in uint32 arithmetic."""
    return (((n & U32) * 2654435761) & U32) ^ (((k & U32) * 40503) & U32) ^ ((k >> 32) & U32) ^ 1


def drift_for_window(state, T, n, k):
    """The trust streak and the drift argument K34 passes to next_window (topk.hip, the
    `next_window(...)` call at the end of the select path of topk_finish_kernel)."""
    valid = state["sh_nk"] == nk_tag(n, k)
    trust = min(state["d_trust"] + 1, 15) if drift_trusted(T, state["t_prev"], state["d_cand"], valid) else 0
    drift = window_drift(T, state["t_prev"], state["d_prev"], valid) if trust >= K_DRIFT_TRUST else 0
    return trust, drift


# ------------------------------------------------------------------------------ fallback prediction
def bucket_counts(skeys, window):
    """G[0..255]: G[j] = #{key >= s_lo + j 2^shift} for j < 255, G[255] = #{key >= s_hi}
    (K2's per-tile suffix counts summed over the tiles; topk.hip "Warm start" comment)."""
    s_lo, s_hi, shift = window[0], window[1], window[2]
    edges = [s_lo + (j << shift) for j in range(K_NMAYBE)] + [s_hi]
    below = np.searchsorted(skeys, np.array(edges, dtype=np.int64), side="left")
    return [int(skeys.size - b) for b in below]


def predict_fallback(skeys, k, window, overflow_word):
    """K34's decision (topk_finish_kernel, `bool fallback = ...` and the kMCap test):
    returns (fallback, G, jstar or None)."""
    G = bucket_counts(skeys, window)
    if overflow_word != 0 or G[0] < k or G[K_NMAYBE] >= k:
        return True, G, None
    jstar = next(j for j in range(K_NMAYBE) if G[j] >= k and G[j + 1] < k)
    if G[jstar] - G[jstar + 1] > K_MCAP:
        return True, G, jstar
    return False, G, jstar


# ------------------------------------------------------------------------------ next window
def _fit(x_lo, x_hi):
    """The smallest shift whose 255 buckets cover [x_lo, x_hi), and the window's ceiling."""
    width = x_hi - x_lo if x_hi > x_lo + K_NMAYBE else K_NMAYBE
    sh = 0
    while (K_NMAYBE << sh) < width:
        sh += 1
    return sh, min(x_lo + (K_NMAYBE << sh), U32)


def warm_m0(k):
    """topk.hip `warm_m0` (host): the margin floor in 1/1024 of k -- kWarmM0, or 8 sigma of the
    sqrt(2 / k) count noise between two independent draws where that is more."""
    m = math.ceil(1024.0 * 8.0 * math.sqrt(2.0 / float(k)))
    return int(min(float(K_WARM_M_MAX), max(float(K_WARM_M0), float(m))))


def next_window(G, window, T, n, k, drift):
    """topk.hip `next_window`: the window the select path prepares for the next call from this
    call's bucket counts.  window = (s_lo, s_hi, shift, m1024) as the call used it.  Returns
    ((s_lo, s_hi, shift, m1024), branches); every fp64 operation in the source's order."""
    s_lo, s_hi, shift, m_prev = window
    kd = float(k)
    br = set()
    m0 = warm_m0(k)
    m = m0
    if m_prev != 0:
        e = max(max(kd * (1.0 + m_prev / 1024.0) - float(G[0]), 0.0),
                max(float(G[K_NMAYBE]) - kd * (1.0 - m_prev / 1024.0), 0.0))
        me = math.ceil(2.0 * e / kd * 1024.0)
        m = int(min(float(K_WARM_M_MAX), max(max(float(m0), float(me)), float(m_prev // 2))))
        if m > m_prev:
            br.add("m_raised")      # (above the floor: a carried window's m_prev is at least the floor)
        elif m < m_prev:
            br.add("m_decayed")
    lo_t = k + k * m // 1024
    hi_t = k - min(k, k * m // 1024)
    nlo = sum(1 for g in G if g >= lo_t)
    nhi = sum(1 for g in G if g > hi_t)
    w0 = s_hi - s_lo
    if nlo >= 1:
        x_lo = s_lo + ((nlo - 1) << shift)
    else:
        br.add("extended_down")
        D, C, need = float((T - s_lo) & U32), float(G[0]) - kd, float(lo_t) - float(G[0])
        dl = 2.0 * D * need / C + float(1 << shift) if C >= max(kd / 1024.0, 16.0) else 2.0 * float(w0) + D
        x_lo = 0 if dl >= float(s_lo) else int(float(s_lo) - dl)
    if nhi <= K_NMAYBE:
        x_hi = min(s_lo + (nhi << shift), s_hi)
    else:
        br.add("extended_up")
        D, C, need = float((s_hi - T) & U32), kd - float(G[K_NMAYBE]), float(G[K_NMAYBE]) - float(hi_t)
        dh = 2.0 * D * need / C + float(1 << shift) if C >= max(kd / 1024.0, 16.0) else 2.0 * float(w0) + D
        x_hi = int(min(float(s_hi) + dh, 2147483648.0))
    if drift != 0:
        br.add("drift_pos" if drift > 0 else "drift_neg")
        lo2, hi2 = x_lo + drift, x_hi + drift
        x_lo = max(0, lo2)
        x_hi = min(2147483648, max(hi2, x_lo + 1))
    sh, w_hi = _fit(x_lo, x_hi)
    if not br:
        br.add("plain")
    return (x_lo & U32, w_hi, sh, m), br


def fallback_window(skeys, n, k):
    """topk.hip `fallback_window`: after the exact fallback, the coarse (key >> 20) bins of the
    keys at the count levels k + k/8 and k - k/8, rounded outward; m1024 = 0."""
    lo_t = min(n, k + k // 8)
    hi_t = max(1, k - k // 8)
    x_lo = (kth_key(skeys, lo_t) >> 20) << 20
    x_hi = ((kth_key(skeys, hi_t) >> 20) + 1) << 20
    width = x_hi - x_lo if x_hi > x_lo + 255 else 255
    sh = 0
    while (K_NMAYBE << sh) < width:
        sh += 1
    return (x_lo, min(x_lo + (K_NMAYBE << sh), U32), sh, 0)


# ------------------------------------------------------------------------------ state step
def step(state, used_window, T_exact, fallback, n, k, prepared=None):
    """The tail of topk_finish_kernel (workgroup 0, thread 0; "Cold backoff" onwards): the ten
    state words after a call that used `used_window`, selected T_exact (ignored after a
    fallback) and prepared the window with edges prepared = (s_lo, s_hi) (select path only).
    Returns (next state, event, backoff_change) with backoff_change in {"doubled", "halved", None}."""
    nk = nk_tag(n, k)
    warm_call = used_window[3] != 0
    bo, cl, hits = state["backoff"], state["cold_left"], state["sh_hits"]
    T = 0 if fallback else T_exact
    shadow_hit = (not fallback) and state["sh_nk"] == nk and state["sh_lo"] <= T < state["sh_hi"]
    change = None
    if warm_call and fallback:
        event = "warm_miss"
        nb = min(max(2 * bo, K_COLD_MIN), K_COLD_MAX)
        if bo != 0 and nb == 2 * bo:
            change = "doubled"
        bo = nb
        cl = bo
        hits = 0
    elif warm_call:
        event = "warm_hit"
        nb = max(bo // 2, K_COLD_MIN)
        if nb < bo:
            change = "halved"
        bo = nb
        hits = 0
    elif cl != 0:
        event = "cold_run_step"
        cl -= 1
        hits = hits + 1 if shadow_hit else 0
        if hits >= K_SHADOW_EXIT:
            event = "shadow_exit"
            cl = 0
            hits = 0
    else:
        event = "cold_call"
    nxt = dict(state)
    nxt["backoff"], nxt["cold_left"], nxt["sh_hits"] = bo, cl, hits
    if not fallback:
        valid = state["sh_nk"] == nk
        trust, _ = drift_for_window(state, T, n, k)
        nxt["d_prev"] = (T - state["t_prev"]) & U32 if (valid and state["t_prev"] != 0) else 0
        nxt["t_prev"] = T
        nxt["sh_lo"], nxt["sh_hi"] = prepared
        nxt["sh_nk"] = nk
        nxt["d_cand"] = window_drift(T, state["t_prev"], state["d_prev"], valid) & U32
        nxt["d_trust"] = trust
    else:
        nxt["t_prev"] = nxt["d_prev"] = nxt["sh_nk"] = nxt["d_cand"] = nxt["d_trust"] = 0
    return nxt, event, change


# ------------------------------------------------------------------------------ host side
def expect_sample(prev, n, k, cold_left_before, fused, warm_enabled, window_before=None):
    """Which sample the call must take: "k1" (the host launches topk_bounds), "k2" (K2's
    prologue samples: the k2_samples word moves) or None.  `prev` is the (n, k) of the previous
    pipeline call on the workspace (None: none), `cold_left_before` the cold-run word before the
    call (the fused step reads its host mirror, which K34 writes on fused calls: pass the word
    as the last *fused* call left it), `window_before` the bounds[par] entry (s_lo, s_hi, shift,
    m1024, n, k, valid) the call finds, when known.  Restates `warm_claim` and `launch_topk`
    (host), and K2's `sample_if_cold && (!ok || cold_left != 0)` rule."""
    warm = prev is not None and prev == (n, k) and warm_enabled
    if fused and warm and cold_left_before != 0:
        warm = False                      # launch_topk: host_cold_left(ws) != 0
    if not warm:
        return "k1"
    if fused:
        return None                       # sample_if_cold = 0: K2 never samples with the fused step
    ok = True
    if window_before is not None:
        w = window_before
        ok = w[6] != 0 and w[4] == n and w[5] == k and w[2] < 32
    return "k2" if (not ok or cold_left_before != 0) else None


# ------------------------------------------------------------------------------ the GPU file's inputs
# One generator for the host and the GPU file: seeded normal deltas (half-normal magnitudes).
# The rates were chosen on an MI355X so that each sequence reaches its named branches
# ("The controller held to a model").
N_FIRST = 65537        # the first n past kSmallN
N_MAIN = 262147
N_LARGE = 1048583
# A scale change of 1 - r moves the count above a fixed key by ~7.5 (1 - r) of k at k = 1 % of
# normal deltas; the margin floor (warm_m0) is 22 % of k at N_MAIN and 11 % at N_LARGE.
SLOW_R = 0.998         # ~1.5 % of k per call: far inside the static window
MEDIUM_R = 0.98        # ~15 % of k per call: inside the window, past half of its margin
MEDIUM_UP_R = 1 / 0.95 # upward the first carried window's ceiling is the sample's (~k / 2 keys above it),
                       # so it takes ~40 % of k per call to push more than k (1 - m) keys past it
FAST_R = 0.95          # ~37 % of k per call: the static window misses
JUMP = 100.0
TIE_STEP = 0.25
TIE_RATIO = 0.5        # at n = 262,147 the k-th of the 1/4-rounded deltas has ~40K equals (> kMCap)


def topk_k(n, ratio):
    """sparsification.py:22,45."""
    return max(1, int(n * (1 - ratio)))


def normal(n, seed):
    return np.random.default_rng(seed).standard_normal(n, dtype=np.float32)


def _call(n, k, x, xhat=None, mem=None, gamma=None, tie=False):
    """One call's inputs and the delta the codec selects on, in the device's fp32 roundings."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    xs = x
    if mem is not None:   # optim/utils.py:67-72: x += gamma * (memory - x_hat), three roundings
        xs = (x + np.float32(gamma) * (mem - xhat).astype(np.float32)).astype(np.float32)
    d = (xs - xhat).astype(np.float32) if xhat is not None else xs
    return {"n": n, "k": k, "x": x, "xhat": xhat, "mem": mem, "gamma": gamma, "d": d, "tie": tie}


def seq_stationary(n, ratio, seed, calls=12, with_xhat=False):
    """Independent redraws; with_xhat: against a fixed x_hat."""
    k = topk_k(n, ratio)
    xhat = (np.float32(0.5) * normal(n, seed + 999)) if with_xhat else None
    for c in range(calls):
        d = normal(n, seed + c)
        yield _call(n, k, (d + xhat).astype(np.float32) if with_xhat else d, xhat)


def seq_drift(n, ratio, seed, r, calls=14, scale0=1.0):
    """One base buffer scaled by scale0 * r^c."""
    k = topk_k(n, ratio)
    base = normal(n, seed)
    for c in range(calls):
        yield _call(n, k, base * np.float32(scale0 * r ** c))


def seq_jump(n, ratio, seed):
    """Scale x JUMP, three stationary calls, x 1/JUMP, three stationary calls, two more (warm
    hits), then x JUMP again directly after a warm hit, and one call of its cold run."""
    k = topk_k(n, ratio)
    scales = [1.0] + [JUMP] * 4 + [1.0] * 6 + [JUMP] * 2
    for c, s in enumerate(scales):
        yield _call(n, k, normal(n, seed + c) * np.float32(s))


def seq_ties(n, seed, calls=4):
    """Deltas rounded to multiples of TIE_STEP: more than kMCap keys equal the k-th."""
    k = topk_k(n, TIE_RATIO)
    for c in range(calls):
        d = np.round(normal(n, seed + c) / np.float32(TIE_STEP)) * np.float32(TIE_STEP)
        yield _call(n, k, d.astype(np.float32), tie=True)


def seq_shapes(seed, calls=8):
    """(n, k) alternating between two shapes (the larger first: one shared workspace)."""
    shapes = [(N_MAIN, topk_k(N_MAIN, 0.99)), (N_FIRST, topk_k(N_FIRST, 0.9))]
    for c in range(calls):
        n, k = shapes[c & 1]
        yield _call(n, k, normal(n, seed + c))


def seq_fused(n, ratio, seed, gamma=0.9):
    """The fused consensus step through a warm miss: stationary (x, memory, x_hat) draws, the
    memory x 1000 from call 2 on; calls 0-4 fused, call 5 without the fused step."""
    k = topk_k(n, ratio)
    for c in range(6):
        x = normal(n, seed + 3 * c)
        xhat = (x + np.float32(0.1) * normal(n, seed + 3 * c + 1)).astype(np.float32)
        mem = (xhat + np.float32(0.05) * normal(n, seed + 3 * c + 2)).astype(np.float32)
        if c >= 2:
            mem = mem * np.float32(1000.0)
        yield _call(n, k, x, xhat, mem, gamma) if c < 5 else _call(n, k, x, xhat)


def seq_fused_after_plain(n, ratio, seed):
    """A cold run started and walked by calls WITHOUT the fused step (which do not write the
    host's mirror of the cold-run word), then fused calls of the same delta scale: the first
    takes the carried window in the middle of the cold run -- a warm hit with a shadow hit
    pending -- and mirrors the cold-run word; the second takes the host-launched K1."""
    k = topk_k(n, ratio)
    for c, s in enumerate([1.0, JUMP, JUMP, JUMP]):
        yield _call(n, k, normal(n, seed + c) * np.float32(s))
    for c in (4, 5):
        xhat = np.float32(0.001) * normal(n, seed + 10 + c)
        x = (normal(n, seed + c) * np.float32(JUMP) + xhat).astype(np.float32)
        yield _call(n, k, x, xhat, xhat.copy(), 0.9)   # memory = x_hat: the consensus step adds 0


def gpu_cases():
    """Every sequence of tests/test_gpu_topk_controller.py: id -> generator factory."""
    cases = {}
    for n in (N_FIRST, N_MAIN, N_LARGE):
        for ratio in (0.9, 0.99):
            for xh in (False, True):
                cases[f"stationary-{n}-{ratio}-{'xhat' if xh else 'plain'}"] = (
                    lambda n=n, ratio=ratio, xh=xh: seq_stationary(n, ratio, 100 + 50 * xh, with_xhat=xh))
    for n in (N_MAIN, N_LARGE):
        cases[f"slow-down-{n}"] = lambda n=n: seq_drift(n, 0.99, 200, SLOW_R)
        cases[f"slow-up-{n}"] = lambda n=n: seq_drift(n, 0.99, 201, 1.0 / SLOW_R)
    # (the medium and fast drifts start where the k-th value, 2.58 sigma, stays inside one binade: a
    # steady scale change is a steady key drift only there)
    cases["medium-down"] = lambda: seq_drift(N_MAIN, 0.99, 250, MEDIUM_R, scale0=1.4)
    cases["medium-up"] = lambda: seq_drift(N_MAIN, 0.99, 251, MEDIUM_UP_R, calls=12, scale0=0.8)
    cases["fast-down"] = lambda: seq_drift(N_MAIN, 0.99, 300, FAST_R, calls=12, scale0=1.5)
    cases["jump"] = lambda: seq_jump(N_MAIN, 0.99, 400)
    cases["ties"] = lambda: seq_ties(N_MAIN, 500)
    cases["shapes"] = lambda: seq_shapes(600)
    cases["warm-off"] = lambda: seq_stationary(N_MAIN, 0.99, 700, calls=5)
    cases["fused"] = lambda: seq_fused(N_MAIN, 0.99, 800)
    cases["fused-after-plain"] = lambda: seq_fused_after_plain(N_MAIN, 0.99, 900)
    return cases
