"""A plain model of the segmented top-k warm path (chocosgd_amd/csrc/topk_seg.hip): the
per-segment windows `SegWin` that `seg_next_window_v` writes from its three histogram
sources, the mode a warm call takes per segment (`seg_bin_kernel`), the cold calls' shadow
checks (`seg_count_kernel`) and the host's warm / cold choice (`seg_claim_warm`).

Python ints and numpy only: no torch, no GPU.  Each function restates one piece of the source
and names it.  tests/test_seg_controller_host.py holds this model to its own contracts;
tests/test_gpu_seg_controller.py holds the device to the model, word by word, after every call.

Assumption (stated once, used everywhere): EVERY CALL IS SYNCHRONISED BEFORE THE NEXT.  The
miss flag a warm call raises is then seen by the very next call (`flag_seen` is "the previous
warm call missed"), and the shadow counter the host reads is the device counter after the
last cold call.  The outputs are exact on every path, so with that assumption the whole
device and host state is a function of the inputs alone and `simulate` runs open loop.

Scope: the multi-tile batched segments (16384 < len <= kSegBatchMax).  A single-tile segment
(ntile == 1) is selected in S2 and has no window; a segment over kSegBatchMax takes the flat
pipeline, which tests/_topk_controller.py models.

All three window sources are restated exactly from the keys, the missed one included: when
`on_T` runs (wide.h, tile 0's phase-3 item, after every phase-2 item is done and before any
workgroup of the segment has left) `hist[0]` holds the select's digit-0 histogram (key >> 20)
and `hist[1]` its digit-1 histogram (bits 19..9 of the keys whose digit 0 is T's) over every
key the reader delivered: the whole segment for kSegMissed, the tiles' candidate lists (the
keys >= the old window's lo) for kSegMissedHigh.
"""
import math

import numpy as np

from _topk_controller import (K_DRIFT_TRUST, U32, _i32, count_ge, drift_trusted, keys, kth_key,  # noqa: F401
                              sorted_keys, topk_k, window_drift)

# topk_seg.hip constants
K_SEG_TILE = 16384                       # kSegTile
K_SEG_BATCH_MAX = K_SEG_TILE * 1024      # kSegBatchMax
K_H = 2048                               # kH
K_WIN_SH_MAX = 9                         # kWinShMax
K_TILE_LIST = 4                          # kTileList
K_SEG_MISS_GAP = 32                      # kSegMissGap
K_SEG_SHADOW_EXIT = 1                    # kSegShadowExit
K_COLD_MIN, K_COLD_MAX = 64, 4096        # the run lengths of seg_claim_warm
K_TRUST_MAX = 15

SELECT, MISSED_LOW, ALL, MISSED_HIGH = 0, 1, 2, 3      # enum SegMode
MODE_NAMES = {SELECT: "select", MISSED_LOW: "missed_low", ALL: "all", MISSED_HIGH: "missed_high"}

WIN_WORDS = ("lo", "sh", "valid", "pad", "t_prev", "d_prev", "cand", "trust")   # struct SegWin
NO_WIN = (0,) * 8                                      # a zero-filled workspace
TAKE_ALL_WIN = (0, K_WIN_SH_MAX, 1, 0, 0, 0, 0, 0)     # seg_emit_w_kernel, mode kSegAll
HOST_WORDS = ("calls", "last_flag", "cold_left", "backoff", "clean", "last_checks", "last_misses")

EVENTS = ("first_call", "warm", "isolated_miss_stays_warm", "recurring_miss_starts_run", "backoff_doubled",
          "cold_run_step", "shadow_exit", "backoff_halved", "cold_run_ran_out")
BRANCHES = ("drift_pos", "drift_neg", "drift_untrusted", "too_wide_centred", "trust_reset", "trust_saturated")
# too_wide_centred cannot be reached: seg_next_window_v takes both edges from ONE histogram of
# kH bins of 2^shb keys (shb <= kWinShMax), so x_hi - x_lo <= kH << shb before the drift, and the
# drift moves both edges alike or clamps one inwards (keys are < 2^31).  The `sh` search therefore
# ends at sh <= shb with the window covered.  The model keeps the branch because the source has it;
# tests/test_seg_controller_host.py proves the bound on every simulated window, and the sequence
# built for it (count levels 12 binades apart) pins what happens instead: the window is the whole
# coarse bin of T.
UNREACHABLE = ("too_wide_centred",)
REQUIRED = tuple(n for n in EVENTS + BRANCHES if n not in UNREACHABLE) + (
    "select", "missed_low", "missed_high", "all", "overflow")


def win_dict(win):
    return dict(zip(WIN_WORDS, win))


# ------------------------------------------------------------------------------ next window
def window_delta(k):
    """seg_next_window_v: delta = (uint64_t)(0.03 k + 4 sqrt(k)) + 8, in double."""
    return int(0.03 * float(k) + 4.0 * math.sqrt(float(k))) + 8


def level_counts(skeys, base, shb, floor=0):
    """C(j) = #{key >= max(base + (j << shb), floor)}, j = 0 .. 2047: what `above + total -
    below` is in seg_next_window_v for each of its callers (skeys ascending, the segment)."""
    edges = np.maximum(base + (np.arange(K_H, dtype=np.int64) << shb), floor)
    return skeys.size - np.searchsorted(skeys, edges, side="left")


def next_window(skeys, base, shb, k, T, old, floor=0):
    """seg_next_window_v + seg_win: the eight SegWin words the call leaves, and the branches
    taken.  `old` is the window whose drift words the caller passes (eight words)."""
    o = win_dict(old)
    br = set()
    delta = window_delta(k)
    lo_t = k + delta
    hi_t = k - delta if k > delta else 0
    C = level_counts(skeys, base, shb, floor)
    nlo = int(np.count_nonzero(C >= lo_t))
    nhi = int(np.count_nonzero(C > hi_t))
    x_lo = base + (((nlo - 1) if nlo else 0) << shb)
    x_hi = base + (nhi << shb)
    valid = o["valid"] != 0
    cand = window_drift(T, o["t_prev"], o["d_prev"], valid)
    trusted = drift_trusted(T, o["t_prev"], o["cand"], valid)
    trust = min(o["trust"] + 1, K_TRUST_MAX) if trusted else 0
    if trusted and o["trust"] + 1 > K_TRUST_MAX:
        br.add("trust_saturated")
    if not trusted and o["trust"] != 0:
        br.add("trust_reset")
    drift = cand if trust >= K_DRIFT_TRUST else 0
    if cand != 0 and drift == 0:
        br.add("drift_untrusted")
    if drift != 0:
        br.add("drift_pos" if drift > 0 else "drift_neg")
        lo2, hi2 = x_lo + drift, x_hi + drift
        x_lo = lo2 if lo2 > 0 else 0
        x_hi = (hi2 if hi2 < (1 << 31) else (1 << 31)) if hi2 > x_lo + 1 else x_lo + 1
    width = (x_hi - x_lo) & 0xFFFFFFFFFFFFFFFF
    sh = 0
    while (K_H << sh) < width and sh < K_WIN_SH_MAX:
        sh += 1
    if (K_H << sh) < width:
        br.add("too_wide_centred")
        sh = K_WIN_SH_MAX
        x_lo = T - (1 << 18) if T > (1 << 18) else 0
    d_prev = (T - o["t_prev"]) & U32 if (valid and o["t_prev"] != 0) else 0
    return (x_lo & U32, sh, 1, 0, T, d_prev, cand & U32, trust), br


def cold_window(skeys, k, T, old):
    """seg_count_kernel (S3b, tile 0): from hist2 of a cold call -- bits 19..9 inside T's
    coarse bin b1, with the keys of the coarse bins above it.  `old`: the window found in
    win[s] before the call."""
    return next_window(skeys, (T >> 20) << 20, 9, k, T, old)


def warm_window(skeys, k, T, win):
    """seg_emit_w_kernel, the segment workgroup (select) and `on_T` on an overflow: from the
    warm hist2, the window's own bins (every candidate key >= lo)."""
    lo, sh = win[0], min(win[1], K_WIN_SH_MAX)
    return next_window(skeys, lo, sh, k, T, win, floor=lo)


def missed_window(skeys, k, T, win, mode):
    """seg_emit_w_kernel `on_T` after a missed window: from the shared select's digit
    histograms -- over the whole segment (kSegMissed) or over the candidates, the keys >= the
    old lo (kSegMissedHigh)."""
    return next_window(skeys, (T >> 20) << 20, 9, k, T, win, floor=win[0] if mode == MISSED_HIGH else 0)


# ------------------------------------------------------------------------------ warm mode
def warm_mode(skeys, k, length, win, ukeys=None):
    """seg_bin_kernel: (mode, overflow, b2, rank) of a warm call that finds `win` -- the mode
    word, whether some tile keeps more than kTileList distinct keys of the k-th key's window
    bin (needs `ukeys`, the segment's keys in element order, for the tile cut), and info words
    3 / 4 (the bin of the k-th key among the candidates' bins, the rank inside it)."""
    lo, sh, valid = win[0], min(win[1], K_WIN_SH_MAX), win[2] != 0
    floor = 0 if k >= length else (lo if valid else U32)      # seg_collect_kernel<WARM>
    shc = sh if valid else 0
    total = count_ge(skeys, floor)
    b2 = rank = 0
    if total >= k:
        T = kth_key(skeys, k)
        b2 = min((T - floor) >> shc, K_H - 1)
        rank = k - (count_ge(skeys, floor + ((b2 + 1) << shc)) if b2 < K_H - 1 else 0)
    if k >= length:
        return ALL, False, b2, rank
    if not valid or total < k:
        return MISSED_LOW, False, b2, rank
    if b2 == K_H - 1:
        return MISSED_HIGH, False, b2, rank
    overflow = False
    if ukeys is not None:
        a, b = lo + (b2 << sh), lo + ((b2 + 1) << sh)
        at = np.nonzero((ukeys >= a) & (ukeys < b))[0]
        tiles = at // K_SEG_TILE
        for t in np.unique(tiles):
            if np.unique(ukeys[at[tiles == t]]).size > K_TILE_LIST:
                overflow = True
    return SELECT, overflow, b2, rank


# ------------------------------------------------------------------------------ shadow check
def shadow_check(T, old):
    """seg_count_kernel `hit`: the window the previous call prepared would have held T."""
    o = win_dict(old)
    return o["valid"] != 0 and o["lo"] <= T < o["lo"] + ((K_H - 1) << min(o["sh"], K_WIN_SH_MAX))


# ------------------------------------------------------------------------------ host
def fresh_host():
    return {w: 0 for w in HOST_WORDS}


def claim(host, flag_seen, shadow_value, nmulti, warm_enabled=True):
    """seg_claim_warm, statement by statement.  `flag_seen`: the pinned miss-flag word is set;
    `shadow_value`: the pinned 64-bit shadow counter (misses << 32 | checks).  Returns
    (warm, new host state, events in the order they happen)."""
    S = dict(host)
    ev = []
    first = S["calls"] == 0
    S["calls"] += 1
    if flag_seen:
        recurring = S["last_flag"] != 0 and S["calls"] - S["last_flag"] <= K_SEG_MISS_GAP
        S["last_flag"] = S["calls"]
        if recurring:
            ev.append("recurring_miss_starts_run")
            nb = min(max(2 * S["backoff"], K_COLD_MIN), K_COLD_MAX)
            if S["backoff"] != 0 and nb == 2 * S["backoff"]:
                ev.append("backoff_doubled")
            S["backoff"] = nb
            S["cold_left"] = nb
            S["last_checks"] = shadow_value & U32
            S["last_misses"] = (shadow_value >> 32) & U32
            S["clean"] = 0
        else:
            ev.append("isolated_miss_stays_warm")
    if first:
        ev.append("first_call")
        return False, S, tuple(ev)
    if S["cold_left"] != 0:
        if nmulti > 0:
            dc = ((shadow_value & U32) - S["last_checks"]) & U32
            dm = (((shadow_value >> 32) & U32) - S["last_misses"]) & U32
            if dc >= nmulti:
                S["clean"] = S["clean"] + dc // nmulti if dm == 0 else 0
                S["last_checks"] = shadow_value & U32
                S["last_misses"] = (shadow_value >> 32) & U32
            if S["clean"] >= K_SEG_SHADOW_EXIT:
                ev.append("shadow_exit")
                S["cold_left"] = 0
                S["clean"] = 0
                if S["backoff"] // 2 >= K_COLD_MIN:
                    ev.append("backoff_halved")
                S["backoff"] = max(S["backoff"] // 2, K_COLD_MIN)
                if warm_enabled:
                    ev.append("warm")
                return warm_enabled, S, tuple(ev)
        S["cold_left"] -= 1
        ev.append("cold_run_step")
        if S["cold_left"] == 0:
            ev.append("cold_run_ran_out")
        return False, S, tuple(ev)
    if warm_enabled:
        ev.append("warm")
    return warm_enabled, S, tuple(ev)


# ------------------------------------------------------------------------------ the whole sequence
def multi_segments(layout):
    """(segment, offset, length) of the segments that carry a window."""
    out, off = [], 0
    for s, m in enumerate(layout):
        if K_SEG_TILE < m <= K_SEG_BATCH_MAX:
            out.append((s, off, m))
        off += m
    return out


def simulate(layout, ratio, sequence, warm_enabled=True):
    """Every call of `sequence` (the fp32 deltas the codec selects on, full length, or the
    dicts of `_call`) on a fresh workspace.  One record per call:
      warm, events, host (HOST_WORDS + flag, as the call leaves them), misses (segments in
      missed_low / missed_high), shadow (the 64-bit counter after the call), reached (names
      of REQUIRED), segs {s: {k, T, source, mode, overflow, found, win, info, branches,
      shadow_hit}} with `found` the window before the call and `win` the one after."""
    multi = multi_segments(layout)
    nmulti = len(multi)
    host, flag, shadow = fresh_host(), 0, 0
    wins = {s: NO_WIN for s, _, _ in multi}
    cache = {}
    log = []
    for item in sequence:
        d = item["d"] if isinstance(item, dict) else item
        if id(d) not in cache:   # (the cache holds d, so the id stays its own)
            uk = keys(d).astype(np.int64)
            cache[id(d)] = (d, {s: (uk[off:off + m], np.sort(uk[off:off + m])) for s, off, m in multi})
        per_seg = cache[id(d)][1]
        warm, host, events = claim(host, flag != 0, shadow, nmulti, warm_enabled)
        flag = 0                 # (seg_claim_warm clears the word it saw)
        reached = set(events)
        segs, misses = {}, 0
        for s, off, m in multi:
            ukeys, skeys = per_seg[s]
            k = topk_k(m, ratio)
            T = kth_key(skeys, min(k, m))
            found = wins[s]
            r = {"k": k, "T": T, "found": found, "overflow": False, "shadow_hit": None, "info": None}
            if not warm:
                r["source"], r["mode"] = "cold", None
                r["shadow_hit"] = shadow_check(T, found)
                shadow += (0 if r["shadow_hit"] else 1 << 32) | 1
                r["win"], r["branches"] = cold_window(skeys, k, T, found)
            else:
                mode, ovf, b2, rank = warm_mode(skeys, k, m, found, ukeys)
                r["mode"], r["overflow"] = mode, ovf
                r["info"] = (found[0], min(found[1], K_WIN_SH_MAX), b2, rank, mode)
                reached.add(MODE_NAMES[mode])
                if mode == ALL:
                    r["source"], r["win"], r["branches"] = "all", TAKE_ALL_WIN, set()
                elif mode == SELECT:
                    r["source"] = "overflow" if ovf else "select"
                    r["win"], r["branches"] = warm_window(skeys, k, T, found)
                    if ovf:
                        reached.add("overflow")
                else:
                    r["source"] = "missed"
                    misses += 1
                    r["win"], r["branches"] = missed_window(skeys, k, T, found, mode)
            reached |= r["branches"]
            wins[s] = r["win"]
            segs[s] = r
        if misses:
            flag = 1
        log.append({"warm": warm, "events": events, "host": dict(host, flag=flag), "misses": misses,
                    "shadow": shadow, "nmulti": nmulti, "reached": reached, "segs": segs})
    return log


# ------------------------------------------------------------------------------ the GPU file's inputs
SMALL = [16385, 40_000, 16384, 5, 7]                     # a 2-tile and a 3-tile segment: nmulti == 2
EDGES = [16385, 131_072, 250_001, 16384, 1, 700_001]     # exact tile multiples, a ragged last tile, 43 tiles
TAKE_ALL = [16385, 5]
DRIFT_G = 1.0 + 3e-5      # ~300 keys per call at the k-th value of normal deltas (a key shift is a
                          # relative change of the value: 2^23 keys per binade)
JUMP_UP, JUMP_DOWN = 100.0, 1e-3
TIE_STEP = 0.125


def normal(n, seed):
    return np.random.default_rng(seed).standard_normal(n, dtype=np.float32)


def _call(x, xhat=None, mem=None, gamma=None):
    """One call's inputs and the delta the codec selects on, in the device's fp32 roundings."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    xs = x
    if mem is not None:   # optim/utils.py:67-72: x += gamma * (memory - x_hat), three roundings
        xs = (x + (np.float32(gamma) * (mem - xhat).astype(np.float32)).astype(np.float32)).astype(np.float32)
    d = (xs - xhat).astype(np.float32) if xhat is not None else xs
    return {"x": x, "xhat": xhat, "mem": mem, "gamma": gamma, "d": d}


def _scaled(layout, seed, scales, kind="plain", hold=False):
    """Fresh normal deltas (hold: the same draw every call), call c scaled by scales[c]; kind
    "xhat": against a fixed x_hat; "gossip": with the fused consensus step (memory near x_hat,
    gamma 0.9)."""
    n = sum(layout)
    xhat = np.float32(0.5) * normal(n, seed + 9999) if kind != "plain" else None
    calls = []
    for c, s in enumerate(scales):
        d = normal(n, seed if hold else seed + c) * np.float32(s)
        if kind == "plain":
            calls.append(_call(d))
        elif kind == "xhat":
            calls.append(_call((d + xhat).astype(np.float32), xhat))
        else:
            mem = (xhat + np.float32(0.05 * s) * normal(n, seed + 5000 + c)).astype(np.float32)
            calls.append(_call((d + xhat).astype(np.float32), xhat, mem, 0.9))
    return calls


def seq_stationary(layout, seed, calls=12, kind="plain"):
    return _scaled(layout, seed, [1.0] * calls, kind)


def seq_drift(layout, seed, gs):
    """One base buffer scaled by the running product of `gs`."""
    base = normal(sum(layout), seed)
    calls, scale = [], 1.0
    for g in gs:
        scale *= g
        calls.append(_call(base * np.float32(scale)))
    return calls


# jump and return: x JUMP_UP (the k-th key above every window: missed-high), hold, x JUMP_DOWN
# (below: missed-low), hold.  The flag of the miss at call c is seen at call c + 1.
JUMP_RECURRING = [1.0] * 3 + [JUMP_UP] * 3 + [JUMP_DOWN] * 4 + [1.0] * 2   # misses 3 calls apart: a cold run, ended
                                                                          # by the first cold call's clean checks
JUMP_ISOLATED = [1.0] * 3 + [JUMP_UP] * 35 + [JUMP_DOWN] * 3               # misses 35 calls apart: never cold
                                                                          # (one draw held: no miss from noise)


def seq_ties(layout, seed):
    """Two calls of normal deltas, two on a 1/8 grid (thousands of equal keys at the k-th: the
    kept-key lists take {key, count}), then normal deltas with, in every multi-tile segment's
    first tile, 32 elements at the keys T - 16 .. T + 16 around the segment's own k-th key T:
    more than kTileList distinct keys in one window bin of one tile (the overflow)."""
    n = sum(layout)
    calls = [_call(normal(n, seed + c)) for c in range(2)]
    for c in (2, 3):
        calls.append(_call((np.round(normal(n, seed + c) / np.float32(TIE_STEP)) * np.float32(TIE_STEP))
                           .astype(np.float32)))
    for c in (4, 5):
        d = normal(n, seed + c)
        for s, off, m in multi_segments(layout):
            seg = d[off:off + m]
            T = kth_key(sorted_keys(seg), topk_k(m, 0.99))
            low = np.argsort(np.abs(seg[:K_SEG_TILE]))[:32]      # the tile's 32 smallest: far below T
            planted = np.array([T + j for j in range(-16, 17) if j != 0], dtype=np.uint32)
            seg[low] = planted.view(np.float32)
        calls.append(_call(d))
    return calls


def seq_too_wide(layout, seed, ratio=0.99, calls=4):
    """In every multi-tile segment the first k_s elements are 4096 (1 + |z|), the rest z: the
    count levels k +- delta lie 12 binades apart, more than 2048 << kWinShMax keys."""
    n = sum(layout)
    out = []
    for c in range(calls):
        d = normal(n, seed + c)
        for s, off, m in multi_segments(layout):
            k = topk_k(m, ratio)
            d[off:off + k] = np.float32(4096.0) * (np.float32(1.0) + np.abs(d[off:off + k]))
        out.append(_call(d))
    return out


def seq_cold_run(layout, seed):
    """a and 2a alternating (the k-th key moves by 2^23 keys each call: outside any window, no
    sign-consistent drift): miss, miss, a run of 64 cold calls whose shadow checks all miss,
    a warm isolated miss, a warm recurring miss (backoff 128), then stationary deltas."""
    n = sum(layout)
    a = normal(n, seed)
    pair = [_call(a), _call(a * np.float32(2.0))]
    calls = [pair[c & 1] for c in range(3 + 64 + 2)]
    last = 1.0 if (len(calls) - 1) & 1 == 0 else 2.0
    calls += _scaled(layout, seed + 1, [last] * 4)
    return calls


def gpu_cases():
    """Every synchronised sequence of tests/test_gpu_seg_controller.py:
    id -> (layout, ratio, warm_enabled, factory of the calls)."""
    c = {}
    c["stationary-small"] = (SMALL, 0.99, True, lambda: seq_stationary(SMALL, 100))
    for ratio in (0.9, 0.99, 0.999):
        c[f"stationary-edges-{ratio}"] = (EDGES, ratio, True, lambda r=ratio: seq_stationary(EDGES, 110))
    c["drift-up"] = (EDGES, 0.99, True, lambda: seq_drift(EDGES, 200, [DRIFT_G] * 8))
    c["drift-down"] = (EDGES, 0.99, True, lambda: seq_drift(EDGES, 201, [1.0 / DRIFT_G] * 8))
    c["drift-long"] = (SMALL, 0.99, True, lambda: seq_drift(SMALL, 202, [DRIFT_G] * 22))
    c["drift-reverses"] = (EDGES, 0.99, True, lambda: seq_drift(EDGES, 203, [DRIFT_G] * 6 + [1.0 / DRIFT_G] * 4))
    c["jump-recurring"] = (EDGES, 0.99, True, lambda: _scaled(EDGES, 300, JUMP_RECURRING))
    c["jump-isolated"] = (SMALL, 0.99, True, lambda: _scaled(SMALL, 310, JUMP_ISOLATED, hold=True))
    c["ties"] = (EDGES, 0.99, True, lambda: seq_ties(EDGES, 400))
    c["too-wide"] = (SMALL, 0.99, True, lambda: seq_too_wide(SMALL, 500))
    c["take-all"] = (TAKE_ALL, 0.0, True, lambda: seq_stationary(TAKE_ALL, 600, calls=4))
    c["cold-run"] = (SMALL, 0.99, True, lambda: seq_cold_run(SMALL, 700))
    c["warm-off"] = (EDGES, 0.99, False, lambda: seq_stationary(EDGES, 800, calls=5))
    c["stationary-xhat"] = (EDGES, 0.99, True, lambda: seq_stationary(EDGES, 900, calls=6, kind="xhat"))
    c["stationary-gossip"] = (EDGES, 0.99, True, lambda: seq_stationary(EDGES, 910, calls=6, kind="gossip"))
    c["jump-xhat"] = (SMALL, 0.99, True, lambda: _scaled(SMALL, 920, JUMP_RECURRING, kind="xhat"))
    c["jump-gossip"] = (SMALL, 0.99, True, lambda: _scaled(SMALL, 930, JUMP_RECURRING, kind="gossip"))
    return c
