"""GPU: the flat top-k warm-start controller (csrc/topk.hip, topk_finish_kernel workgroup 0
and launch_topk) held to the plain model of tests/_topk_controller.py after EVERY call:
fallback taken, sample source, window used, window prepared and all ten state words, as
exact integers.  The outputs are exact on every path, so only the control block shows
whether the drift, the shadow exit, the backoff and the margin rule still do what they say.
Run on an MI355X with `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import _topk_controller as M
from conftest import same_bits
from oracle import choco_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = M.gpu_cases()   # the inputs, shared with tests/test_topk_controller_host.py

# the events, next_window branches and backoff moves the sequences of this file went through
REACHED = set()
REQUIRED = ["warm_hit", "warm_miss", "cold_run_step", "shadow_exit", "cold_call", "backoff doubled",
            "backoff halved", "drift_pos", "drift_neg", "m_raised", "m_decayed", "extended_down", "extended_up"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def _word(off):
    from chocosgd_amd import codec
    return codec.topk_workspace_word(off) & 0xFFFFFFFF


def _window(par):
    """bounds[par]: (s_lo, s_hi, shift, m1024, n, k, valid)."""
    from chocosgd_amd import _lib as L
    b = L.TOPK_DIAG_BOUNDS_OFFSET + L.TOPK_DIAG_BOUNDS_STRIDE * par
    w32 = [_word(b + o) for o in (L.TOPK_DIAG_BOUNDS_S_LO, L.TOPK_DIAG_BOUNDS_S_HI, L.TOPK_DIAG_BOUNDS_SHIFT,
                                  L.TOPK_DIAG_BOUNDS_M1024)]
    n = _word(b + L.TOPK_DIAG_BOUNDS_N) | (_word(b + L.TOPK_DIAG_BOUNDS_N + 4) << 32)
    k = _word(b + L.TOPK_DIAG_BOUNDS_K) | (_word(b + L.TOPK_DIAG_BOUNDS_K + 4) << 32)
    return tuple(w32) + (n, k, _word(b + L.TOPK_DIAG_BOUNDS_VALID))


def _state():
    from chocosgd_amd import _lib as L
    offs = {"t_prev": L.TOPK_DIAG_T_PREV_OFFSET, "d_prev": L.TOPK_DIAG_D_PREV_OFFSET,
            "sh_lo": L.TOPK_DIAG_SH_LO_OFFSET, "sh_hi": L.TOPK_DIAG_SH_HI_OFFSET, "sh_nk": L.TOPK_DIAG_SH_NK_OFFSET,
            "sh_hits": L.TOPK_DIAG_SH_HITS_OFFSET, "d_cand": L.TOPK_DIAG_D_CAND_OFFSET,
            "d_trust": L.TOPK_DIAG_D_TRUST_OFFSET, "backoff": L.TOPK_DIAG_BACKOFF_OFFSET,
            "cold_left": L.TOPK_COLD_LEFT_OFFSET}
    return {w: _word(offs[w]) for w in M.STATE_WORDS}


def run_sequence(calls, warm=True):
    """Drive `calls` (dicts of tests/_topk_controller._call) through codec.topk on a fresh
    workspace and hold every call to the model.  Returns one record per call."""
    from chocosgd_amd import _lib as L, codec
    torch.cuda.synchronize()
    codec.release_workspaces()   # call parity starts at 0, the host's map is empty
    state = M.fresh_state()
    prev_shape, prev_prepared, mirror = None, None, 0
    log = []
    for c, call in enumerate(calls):
        n, k, par = call["n"], call["k"], c & 1
        fused = call["mem"] is not None
        at = f"call {c} (n={n}, k={k})"
        # ---- 1. before
        cold_before = _word(L.TOPK_COLD_LEFT_OFFSET)
        assert cold_before == state["cold_left"], at
        k1_0, s_0, f_0 = codec.launch_count("topk_bounds"), _word(L.TOPK_K2_SAMPLES_OFFSET), \
            _word(L.TOPK_FALLBACKS_OFFSET)
        found = _window(par) if c > 0 else None
        # ---- 2. the call, exact against the oracle
        x = dev(call["x"])
        xh = dev(call["xhat"]) if call["xhat"] is not None else None
        if fused:
            vals, idx = codec.topk(x, k, xhat=xh, gossip=(dev(call["mem"]), call["gamma"]))
            assert same_bits(host(x), O.gossip_step(call["x"], call["mem"], call["xhat"], call["gamma"])), at
        else:
            vals, idx = codec.topk(x, k, xhat=xh)
        torch.cuda.synchronize()
        ov, oi = O.topk(call["d"], k)
        assert np.array_equal(host(idx).astype(np.int64), oi), at
        assert same_bits(host(vals), ov), at
        # ---- 3. after
        used, prepared, ovf = _window(par), _window(par ^ 1), _word(L.TOPK_DIAG_OVERFLOW_OFFSET + 4 * par)
        after = _state()
        fell = _word(L.TOPK_FALLBACKS_OFFSET) - f_0
        k1 = codec.launch_count("topk_bounds") - k1_0
        k2 = _word(L.TOPK_K2_SAMPLES_OFFSET) - s_0
        assert (k1, k2) in ((1, 0), (0, 1), (0, 0)), (at, k1, k2)
        sample = "k1" if k1 else ("k2" if k2 else None)
        # ---- 4. the model
        skeys = M.sorted_keys(call["d"])
        T = M.kth_key(skeys, k)
        assert used[4:] == (n, k, 1), (at, used)
        want_fb, G, _ = M.predict_fallback(skeys, k, used, ovf)
        assert bool(fell) == want_fb and fell in (0, 1), (at, fell, want_fb, used, ovf)
        assert sample == M.expect_sample(prev_shape, n, k, mirror if fused else cold_before, fused, warm, found), at
        if sample is None:
            assert used == prev_prepared, (at, used, prev_prepared)
        else:
            assert used[3] == 0, (at, used)   # a sampled window carries no margin
        if want_fb:
            want_win, branches = M.fallback_window(skeys, n, k), {"fallback"}
            want_state, event, change = M.step(state, used, T, True, n, k)
        else:
            _, drift = M.drift_for_window(state, T, n, k)
            want_win, branches = M.next_window(G, used[:4], T, n, k, drift)
            want_state, event, change = M.step(state, used, T, False, n, k, prepared=want_win[:2])
            assert (after["sh_lo"], after["sh_hi"]) == prepared[:2], at
        assert prepared == want_win + (n, k, 1), (at, event, branches, prepared, want_win)
        assert after == want_state, (at, event, after, want_state)
        assert _word(L.TOPK_STATUS_OFFSET) == 0, at
        # ---- 5. record
        REACHED.add(event)
        REACHED.update(branches)
        if change:
            REACHED.add("backoff " + change)
        log.append({"event": event, "branches": branches, "change": change, "sample": sample, "fallback": want_fb,
                    "used": used, "prepared": prepared, "state": after, "T": T})
        state, prev_shape, prev_prepared = want_state, (n, k), prepared
        if fused:
            mirror = after["cold_left"]   # K34 mirrors the cold-run word to the host on fused calls only
    return log


def _events(log):
    return [r["event"] for r in log]


# ------------------------------------------------------------------------------ stationary
@pytest.mark.parametrize("with_xhat", [False, True], ids=["plain", "xhat"])
@pytest.mark.parametrize("ratio", [0.9, 0.99])
@pytest.mark.parametrize("n", [M.N_FIRST, M.N_MAIN, M.N_LARGE])
def test_stationary(n, ratio, with_xhat):
    """12 independent redraws: K1 on call 1 only, no fallback, the margin stays at its floor on
    every prepared window and no cold run starts."""
    log = run_sequence(CASES[f"stationary-{n}-{ratio}-{'xhat' if with_xhat else 'plain'}"]())
    print([(r["event"], r["prepared"][3], r["state"]["cold_left"]) for r in log])
    assert [r["sample"] for r in log] == ["k1"] + [None] * 11
    assert not any(r["fallback"] for r in log)
    assert all(r["prepared"][3] == M.warm_m0(r["prepared"][5]) for r in log)
    assert all(r["state"]["cold_left"] == 0 for r in log)
    assert _events(log) == ["cold_call"] + ["warm_hit"] * 11


# ------------------------------------------------------------------------------ slow steady drift
@pytest.mark.parametrize("up", [False, True], ids=["down", "up"])
@pytest.mark.parametrize("n", [M.N_MAIN, M.N_LARGE])
def test_slow_drift(n, up):
    """One buffer scaled by SLOW_R^c (or its inverse): the drift is trusted after kDriftTrust
    confirmations and from then on the prepared window is the undrifted one moved by d_cand
    (the next_window equality of run_sequence, with the model's drift argument); no fallback."""
    log = run_sequence(CASES[f"slow-{'up' if up else 'down'}-{n}"]())
    print([(r["event"], sorted(r["branches"]), r["prepared"][3], r["state"]["d_trust"]) for r in log])
    assert not any(r["fallback"] for r in log)
    trust = [r["state"]["d_trust"] for r in log]
    first = next(c for c, t in enumerate(trust) if t >= M.K_DRIFT_TRUST)
    assert first <= 5 and all(t >= M.K_DRIFT_TRUST for t in trust[first:])
    tag = "drift_pos" if up else "drift_neg"
    for r in log[first:]:
        assert tag in r["branches"]
        d = r["state"]["d_cand"]
        assert d != 0 and (d < 0x80000000) == up


# ------------------------------------------------------------------------------ medium steady drift
@pytest.mark.parametrize("up", [False, True], ids=["down", "up"])
def test_medium_drift(up):
    """A drift that stays inside the carried window but comes closer to an edge than half of
    the margin: no fallback; the margin is raised and decays again once the drift is followed
    (down), the window is extended past the edge the keys ran over (down: the floor, up: the
    ceiling)."""
    log = run_sequence(CASES["medium-up" if up else "medium-down"]())
    print([(r["event"], sorted(r["branches"]), r["prepared"][3]) for r in log])
    assert not any(r["fallback"] for r in log)
    seen = set().union(*(r["branches"] for r in log))
    assert ({"extended_up", "drift_pos"} if up else {"extended_down", "m_raised", "m_decayed", "drift_neg"}) <= seen
    m0 = M.warm_m0(log[0]["prepared"][5])
    assert all(m0 <= r["prepared"][3] <= M.K_WARM_M_MAX for r in log) and log[-1]["prepared"][3] == m0


# ------------------------------------------------------------------------------ fast steady drift
def test_fast_drift():
    """The static window misses on the first warm call: a cold run of backoff = 64 calls that
    sample in K2 (no K1), ended by the shadow exit once the drift-moved windows held the k-th
    key kShadowExit calls in a row -- not by counting down."""
    log = run_sequence(CASES["fast-down"]())
    ev = _events(log)
    print(list(zip(ev, [r["state"]["cold_left"] for r in log])))
    assert ev[:2] == ["cold_call", "warm_miss"]
    assert log[1]["state"]["cold_left"] == log[1]["state"]["backoff"] == 64
    x = ev.index("shadow_exit")
    assert ev[2:x] == ["cold_run_step"] * (x - 2)
    assert all(r["sample"] == "k2" for r in log[2:x + 1])
    assert log[x - 1]["state"]["cold_left"] > 0 and log[x]["state"]["cold_left"] == 0
    assert "drift_neg" in log[x]["branches"]
    assert ev[x + 1:] == ["warm_hit"] * (len(ev) - x - 1) and len(ev) > x + 1
    assert sum(r["fallback"] for r in log) == 1


# ------------------------------------------------------------------------------ jump and return
def test_jump_and_return():
    """x JUMP, three stationary calls, x 1/JUMP, three stationary calls, warm hits, x JUMP
    directly after a warm hit: the backoff is 64 on the first miss, 128 on the next run's miss
    (no warm hit between), halved -- not below 64 -- by warm hits, doubled again by the miss
    after them; t_prev, d_prev, sh_nk, d_cand, d_trust are zero after each fallback."""
    log = run_sequence(CASES["jump"]())
    ev = _events(log)
    print(list(zip(ev, [(r["state"]["backoff"], r["state"]["cold_left"]) for r in log])))
    assert ev == ["cold_call", "warm_miss", "cold_run_step", "cold_run_step", "shadow_exit",
                  "warm_miss", "cold_run_step", "cold_run_step", "shadow_exit",
                  "warm_hit", "warm_hit", "warm_miss", "cold_run_step"]
    assert [r["state"]["backoff"] for r in log] == [0, 64, 64, 64, 64, 128, 128, 128, 128, 64, 64, 128, 128]
    assert [r["change"] for r in log if r["change"]] == ["doubled", "halved", "doubled"]
    for r in log:
        if r["fallback"]:
            assert all(r["state"][w] == 0 for w in ("t_prev", "d_prev", "sh_nk", "d_cand", "d_trust", "sh_hits"))
            assert r["state"]["cold_left"] == r["state"]["backoff"]


# ------------------------------------------------------------------------------ ties
def test_ties_fall_back_on_the_bucket_count():
    """Deltas rounded to multiples of 1/4: more than kMCap keys equal the k-th, so the bucket
    that holds it cannot be selected in LDS, whatever the window."""
    calls = list(CASES["ties"]())
    log = run_sequence(calls)
    for call, r in zip(calls, log):
        skeys = M.sorted_keys(call["d"])
        assert M.count_ge(skeys, r["T"]) - M.count_ge(skeys, r["T"] + 1) > M.K_MCAP
        assert r["fallback"] and r["event"] == "cold_call" and r["prepared"][3] == 0
        if r["used"][0] <= r["T"] < r["used"][1]:   # a window that holds the key: the bucket count alone decides
            assert M.predict_fallback(skeys, call["k"], r["used"], 0)[0]
    assert any(r["used"][0] <= r["T"] < r["used"][1] for r in log)


# ------------------------------------------------------------------------------ shape change
def test_shape_change_is_a_cold_call():
    """(n, k) alternating on the shared workspace: every call takes K1 and starts its drift
    words from nothing (sh_nk is the other shape's)."""
    log = run_sequence(CASES["shapes"]())
    assert [r["sample"] for r in log] == ["k1"] * len(log)
    assert _events(log) == ["cold_call"] * len(log)
    assert all(r["state"]["d_prev"] == 0 and r["state"]["d_cand"] == 0 and r["state"]["d_trust"] == 0 for r in log)
    assert len({r["state"]["sh_nk"] for r in log}) == 2


# ------------------------------------------------------------------------------ warm start off
def test_warm_start_off_samples_every_call():
    from chocosgd_amd import codec
    lib = codec.lib()
    lib.choco_topk_set_warm_start(0)
    try:
        log = run_sequence(CASES["warm-off"](), warm=False)
    finally:
        lib.choco_topk_set_warm_start(1)
    assert [r["sample"] for r in log] == ["k1"] * 5
    assert all(r["used"][3] == 0 for r in log)
    assert _events(log) == ["cold_call"] * 5
    assert all(r["state"]["t_prev"] == r["T"] for r in log)   # the state words are still tracked
    assert all(r["state"]["d_prev"] != 0 for r in log[1:])


# ------------------------------------------------------------------------------ fused consensus step
def test_fused_gossip_cold_run_takes_host_k1():
    """test_topk_fused_gossip_cold_run_takes_host_k1 (test_gpu_topk.py, 25M) at n = 262,147 with
    every call held to the model: a warm miss of a fused call starts a cold run; the fused
    calls on it take the host-launched K1 and K2's sample counter does not move; the same cold
    run without the fused step samples in K2."""
    log = run_sequence(CASES["fused"]())
    ev = _events(log)
    print(list(zip(ev, [r["sample"] for r in log])))
    assert ev[:3] == ["cold_call", "warm_hit", "warm_miss"]
    assert [r["sample"] for r in log] == ["k1", None, None, "k1", "k1", "k2"]
    assert all(e in ("cold_run_step", "shadow_exit") for e in ev[3:5])
    assert log[4]["state"]["cold_left"] > 0   # call 5 is still on the cold run


def test_fused_call_in_a_cold_run_the_host_has_not_seen():
    """Only fused calls mirror the cold-run word to the host.  A cold run started by calls
    without the fused step is invisible to a fused call's host side: it takes the carried
    window (K2 never samples with the fused step) -- here a warm hit in the middle of the cold
    run, which clears the pending shadow hit, halves nothing below 64, leaves cold_left alone
    and mirrors it, so that the next fused call runs K1."""
    log = run_sequence(CASES["fused-after-plain"]())
    ev = _events(log)
    print(list(zip(ev, [r["sample"] for r in log], [(r["state"]["sh_hits"], r["state"]["cold_left"]) for r in log])))
    assert ev == ["cold_call", "warm_miss", "cold_run_step", "cold_run_step", "warm_hit", "cold_run_step"]
    assert [r["sample"] for r in log] == ["k1", None, "k2", "k2", None, "k1"]
    assert [r["state"]["sh_hits"] for r in log[2:]] == [0, 1, 0, 1]
    assert [r["state"]["cold_left"] for r in log[1:]] == [64, 63, 62, 62, 61]


# ------------------------------------------------------------------------------ reached branches
def test_every_named_branch_was_reached():
    """Needs the whole file to have run: every event, both backoff moves, both drift signs, the
    margin raised and decayed, and both window extensions occurred in some sequence above."""
    missing = [b for b in REQUIRED if b not in REACHED]
    assert not missing, (missing, sorted(REACHED))
