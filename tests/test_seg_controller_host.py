"""CPU: the model of the segmented top-k warm path (tests/_seg_controller.py) held to its own
contracts, and the proof that the sequences tests/test_gpu_seg_controller.py runs reach every
named event, window branch and warm mode by the model alone.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _seg_controller as S
from conftest import ROOT

CASES = S.gpu_cases()


@pytest.fixture(scope="module")
def logs():
    """Every GPU sequence, simulated once: id -> (layout, ratio, calls, records)."""
    out = {}
    for name, (layout, ratio, warm_enabled, make) in CASES.items():
        calls = make()
        out[name] = (layout, ratio, calls, S.simulate(layout, ratio, calls, warm_enabled))
    return out


def _events(log):
    return [r["events"] for r in log]


# ------------------------------------------------------------------------------ next_window
def test_window_properties(logs):
    """Every window `simulate` produces on the GPU sequences: sh <= kWinShMax, trust <= 15, the
    floor keeps at least k keys of the call's own data (C(lo) >= k: the drifts applied here,
    ~300 keys, are far inside the delta margin), a window written without drift holds the
    call's own T, and t_prev is that call's T whatever the source."""
    seen = 0
    for name, (layout, ratio, calls, log) in logs.items():
        for call, rec in zip(calls, log):
            for s, off, m in S.multi_segments(layout):
                r = rec["segs"][s]
                if r["source"] == "all":
                    assert r["win"] == S.TAKE_ALL_WIN
                    continue
                w = S.win_dict(r["win"])
                skeys = S.sorted_keys(call["d"][off:off + m])
                at = (name, s, r["source"], w)
                assert w["valid"] == 1 and w["pad"] == 0, at
                assert w["sh"] <= S.K_WIN_SH_MAX, at
                assert w["trust"] <= S.K_TRUST_MAX, at
                assert w["t_prev"] == r["T"], at
                assert S.count_ge(skeys, w["lo"]) >= r["k"], at
                if not r["branches"] & {"drift_pos", "drift_neg"}:
                    assert w["lo"] <= r["T"] < w["lo"] + (S.K_H << w["sh"]), at
                seen += 1
    assert seen > 500


def test_window_width_is_bounded_by_its_histogram(logs):
    """Why too_wide_centred is not in REQUIRED: before the `sh` search the window spans at
    most kH << shb keys, whatever the keys are, so the search never runs out.  Checked on every
    simulated window and on count levels 12 binades apart."""
    for name, (layout, ratio, calls, log) in logs.items():
        assert not any("too_wide_centred" in r["reached"] for r in log), name
    rng = np.random.default_rng(1)
    z = np.abs(rng.standard_normal(40_000, dtype=np.float32))
    z[:400] = 4096.0 * (1.0 + z[:400])
    skeys = S.sorted_keys(z)
    T = S.kth_key(skeys, 400)
    win, br = S.cold_window(skeys, 400, T, S.NO_WIN)
    assert "too_wide_centred" not in br
    assert (win[0], win[1]) == ((T >> 20) << 20, S.K_WIN_SH_MAX)   # the whole coarse bin of T
    for r in logs["too-wide"][3][0]["segs"].values():     # the GPU sequence built for it: its cold call
        assert (r["win"][0], r["win"][1]) == ((r["T"] >> 20) << 20, S.K_WIN_SH_MAX)


def test_window_delta_terms():
    """delta = int(0.03 k + 4 sqrt(k)) + 8 at the three ratios of the GPU file: dominated in
    turn by 0.03 k, 4 sqrt(k) and + 8; and at no k of the GPU layouts would a fused multiply-add
    on the device (0.03 k unrounded into the sum) truncate to another integer."""
    from fractions import Fraction
    assert S.window_delta(70_000) == 2100 + 1058 + 8 and 0.03 * 70_000 > 4 * 70_000 ** 0.5
    assert S.window_delta(163) == 4 + 51 + 8 and 4 * 163 ** 0.5 > max(0.03 * 163, 8)
    assert S.window_delta(1) == 4 + 8 and 8 > 0.03 + 4
    for layout, ratio, _, _ in CASES.values():
        for _, _, m in S.multi_segments(layout):
            k = S.topk_k(m, ratio)
            root = 4.0 * math.sqrt(float(k))
            fused = float(Fraction(0.03) * k + Fraction(root))
            assert int(fused) == int(0.03 * float(k) + root), (m, ratio, k)


def test_next_window_drift_rules():
    """Hand-worked: the drift needs two moves of one sign to be proposed and kDriftTrust
    confirmations to be applied; a reversal proposes nothing and resets the streak."""
    skeys = np.arange(1 << 20, (1 << 20) + 100_000, dtype=np.int64) * 8
    k = 1000

    def step(T, old):
        return S.next_window(skeys, (T >> 20) << 20, 9, k, T, old)

    T0 = S.kth_key(skeys, k)
    w, br = step(T0, S.NO_WIN)
    assert w[4:] == (T0, 0, 0, 0) and not br
    w, br = step(T0 + 300, w)                  # first move: d_prev, nothing proposed
    assert w[4:] == (T0 + 300, 300, 0, 0) and not br
    w, br = step(T0 + 600, w)                  # second move, same sign: proposed, no streak yet
    assert w[4:] == (T0 + 600, 300, 300, 0) and br == {"drift_untrusted"}
    plain_lo = w[0]
    w, br = step(T0 + 900, w)                  # the proposal predicted it: streak 1
    assert w[4:] == (T0 + 900, 300, 300, 1) and br == {"drift_untrusted"} and w[0] == plain_lo
    w, br = step(T0 + 1200, w)                 # streak 2: applied, both edges move
    assert w[4:] == (T0 + 1200, 300, 300, 2) and br == {"drift_pos"} and w[0] == plain_lo + 300
    w, br = step(T0 + 1000, w)                 # reversal
    assert w[4:] == (T0 + 1000, (-200) & S.U32, 0, 0) and br == {"trust_reset"} and w[0] == plain_lo


def test_shadow_check_is_the_clamped_window():
    """The hit test leaves the clamped top bin out (a k-th key there is a missed-high call)."""
    w = (1000, 3, 1, 0, 0, 0, 0, 0)
    assert S.shadow_check(1000, w) and S.shadow_check(1000 + (2047 << 3) - 1, w)
    assert not S.shadow_check(999, w) and not S.shadow_check(1000 + (2047 << 3), w)
    assert not S.shadow_check(1000, S.NO_WIN)
    assert S.shadow_check(5 + (2047 << 9) - 1, (5, 12, 1, 0, 0, 0, 0, 0))   # sh is clamped to kWinShMax


# ------------------------------------------------------------------------------ claim
def _run_claims(miss_calls, ncalls, shadow_miss=True, nmulti=2):
    """Drive `claim` alone: warm calls listed in `miss_calls` (0-based) miss when they run warm;
    every cold call adds nmulti shadow checks, all misses or all hits."""
    host, flag, shadow, out = S.fresh_host(), False, 0, []
    for c in range(ncalls):
        warm, host, ev = S.claim(host, flag, shadow, nmulti)
        flag = False
        if warm:
            flag = c in miss_calls
        else:
            shadow += ((nmulti << 32) if shadow_miss else 0) | nmulti
        out.append((warm, ev, dict(host)))
    return out


def test_claim_isolated_misses_stay_warm():
    """Misses at calls 3 and 40 (seen at 4 and 41, gap 37 > kSegMissGap): both isolated."""
    out = _run_claims({3, 40}, 45)
    assert [w for w, _, _ in out] == [False] + [True] * 44
    assert [c for c, (_, ev, _) in enumerate(out) if "isolated_miss_stays_warm" in ev] == [4, 41]
    assert all(h["cold_left"] == 0 and h["backoff"] == 0 for _, _, h in out)
    assert out[-1][2]["last_flag"] == 42


def test_claim_recurring_miss_starts_a_run_of_64():
    """Misses at calls 3 and 20 (gap 17): the second starts a run of 64 cold calls, which runs
    out (every shadow check misses) and hands back to warm."""
    out = _run_claims({3, 20}, 90)
    assert "isolated_miss_stays_warm" in out[4][1] and "recurring_miss_starts_run" in out[21][1]
    assert out[21][2]["backoff"] == 64 and out[21][2]["cold_left"] == 63
    assert [w for w, _, _ in out[21:85]] == [False] * 64
    assert "cold_run_ran_out" in out[84][1] and out[84][2]["cold_left"] == 0
    assert out[85][0] and out[85][1] == ("warm",)


def test_claim_backoff_doubles_to_4096_and_halves_to_64():
    """Runs that end in a new miss double: 64, 128, ... capped at 4096; an exit halves, not
    below 64."""
    host, shadow, runs = S.fresh_host(), 0, []
    _, host, _ = S.claim(host, False, shadow, 2)
    _, host, ev = S.claim(host, True, shadow, 2)
    assert ev == ("isolated_miss_stays_warm", "warm") and host["backoff"] == 0
    for i in range(9):
        _, host, ev = S.claim(host, True, shadow, 2)     # a miss seen within kSegMissGap of the last
        assert "recurring_miss_starts_run" in ev and ("backoff_doubled" in ev) == (1 <= i <= 6)
        runs.append(host["backoff"])
        assert host["cold_left"] == host["backoff"] - 1
        host["cold_left"] = 0                            # (the run's other calls, skipped)
    assert runs == [64, 128, 256, 512, 1024, 2048, 4096, 4096, 4096]
    halves = []
    for _ in range(8):
        host["cold_left"] = 5
        shadow += 2                                      # one cold call's checks, no miss
        warm, host, ev = S.claim(host, False, shadow, 2)
        assert warm and "shadow_exit" in ev and host["cold_left"] == 0 and host["clean"] == 0
        assert ("backoff_halved" in ev) == (halves[-1] > 64 if halves else True)
        halves.append(host["backoff"])
    assert halves == [2048, 1024, 512, 256, 128, 64, 64, 64]


def test_claim_checks_from_before_the_run_do_not_count():
    """The shadow counter is re-based when a run starts, a dirty cold call zeroes `clean`, and
    warm start off keeps every call cold without touching the run."""
    host = dict(S.fresh_host(), calls=10, last_flag=9)
    warm, host, ev = S.claim(host, True, (7 << 32) | 40, 2)
    assert not warm and ev == ("recurring_miss_starts_run", "cold_run_step")
    assert (host["last_checks"], host["last_misses"], host["clean"], host["cold_left"]) == (40, 7, 0, 63)
    warm, host, ev = S.claim(host, False, (8 << 32) | 42, 2)     # that cold call's checks: one miss
    assert not warm and host["clean"] == 0 and (host["last_checks"], host["last_misses"]) == (42, 8)
    warm, host, ev = S.claim(host, False, (8 << 32) | 43, 2)     # half a call's checks: nothing moves
    assert not warm and (host["last_checks"], host["clean"], host["cold_left"]) == (42, 0, 61)
    warm, host, ev = S.claim(host, False, (8 << 32) | 44, 2, warm_enabled=False)
    assert not warm and ev == ("shadow_exit",) and host["cold_left"] == 0 and host["backoff"] == 64


# ------------------------------------------------------------------------------ the sequences
def test_stationary_is_warm_without_a_miss(logs):
    for name in ("stationary-small", "stationary-edges-0.99", "stationary-xhat", "stationary-gossip"):
        log = logs[name][3]
        assert [r["warm"] for r in log] == [False] + [True] * (len(log) - 1), name
        assert all(r["misses"] == 0 for r in log), name
        assert all(v["source"] == "select" for r in log[1:] for v in r["segs"].values()), name
        assert all(v["win"][7] <= 1 for r in log for v in r["segs"].values()), name    # no streak builds


def test_drift_sequences(logs):
    for name, tag in (("drift-up", "drift_pos"), ("drift-down", "drift_neg")):
        log = logs[name][3]
        assert all(r["misses"] == 0 for r in log)
        for s in log[0]["segs"]:
            trust = [r["segs"][s]["win"][7] for r in log]
            assert trust == [0, 0, 0, 1, 2, 3, 4, 5], (name, s, trust)
            for r in log[4:]:
                vb = r["segs"][s]
                assert tag in vb["branches"]
                d = S._i32(vb["win"][6])
                assert d != 0 and (d > 0) == (tag == "drift_pos")
    log = logs["drift-long"][3]
    assert all(v["win"][7] == S.K_TRUST_MAX for v in log[-1]["segs"].values())
    log = logs["drift-reverses"][3]
    for s in log[0]["segs"]:
        v = log[6]["segs"][s]                  # the first call after the reversal
        assert "trust_reset" in v["branches"] and not v["branches"] & {"drift_pos", "drift_neg"}
        assert v["win"][6] == 0 and v["win"][7] == 0


def test_jump_sequences(logs):
    log = logs["jump-isolated"][3]
    assert [r["warm"] for r in log] == [False] + [True] * 40
    assert [c for c, r in enumerate(log) if r["misses"]] == [3, 38]
    assert {v["mode"] for v in log[3]["segs"].values()} == {S.MISSED_HIGH}
    assert {v["mode"] for v in log[38]["segs"].values()} == {S.MISSED_LOW}
    assert sum("isolated_miss_stays_warm" in r["events"] for r in log) == 2
    for name in ("jump-recurring", "jump-xhat", "jump-gossip"):
        log = logs[name][3]
        assert log[3]["misses"] and log[6]["misses"], name
        assert "recurring_miss_starts_run" in log[7]["events"] and not log[7]["warm"], name
        assert "shadow_exit" in log[8]["events"] and log[8]["warm"], name   # one clean cold call ends the run
        assert log[8]["host"]["backoff"] == 64 and log[8]["host"]["cold_left"] == 0, name


def test_ties_overflow_is_not_a_miss(logs):
    log = logs["ties"][3]
    assert any(v["overflow"] for v in log[4]["segs"].values()) and log[4]["misses"] == 0
    assert all(v["overflow"] for v in log[5]["segs"].values()) and log[5]["misses"] == 0
    for r in log[4:]:
        for v in r["segs"].values():
            if v["overflow"]:
                assert v["mode"] == S.SELECT and v["source"] == "overflow"


def test_take_all_window(logs):
    log = logs["take-all"][3]
    assert [v["mode"] for r in log[1:] for v in r["segs"].values()] == [S.ALL] * 3
    assert all(v["win"] == S.TAKE_ALL_WIN for r in log[1:] for v in r["segs"].values())


def test_cold_run_runs_out_doubles_and_exits(logs):
    log = logs["cold-run"][3]
    ev = _events(log)
    assert [r["warm"] for r in log[:3]] == [False, True, True] and log[1]["misses"] == log[2]["misses"] == 2
    assert ev[2] == ("isolated_miss_stays_warm", "warm")
    assert ev[3] == ("recurring_miss_starts_run", "cold_run_step")
    assert ev[4:66] == [("cold_run_step",)] * 62 and ev[66] == ("cold_run_step", "cold_run_ran_out")
    assert all(not v["shadow_hit"] for r in log[3:67] for v in r["segs"].values())
    assert ev[67] == ("warm",) and ev[68] == ("isolated_miss_stays_warm", "warm")
    assert ev[69] == ("recurring_miss_starts_run", "backoff_doubled", "cold_run_step")
    assert (log[69]["host"]["backoff"], log[69]["host"]["cold_left"]) == (128, 127)
    assert ev[70] == ("shadow_exit", "backoff_halved", "warm") and log[70]["host"]["backoff"] == 64
    assert all(r["warm"] and not r["misses"] for r in log[70:])


def test_warm_start_off_is_cold_every_call(logs):
    log = logs["warm-off"][3]
    assert not any(r["warm"] for r in log)
    assert [r["shadow"] & S.U32 for r in log] == [4 * (c + 1) for c in range(5)]
    assert log[0]["shadow"] >> 32 == 4 and all(r["host"]["cold_left"] == 0 for r in log)


def test_gpu_sequences_reach_every_required_name(logs):
    """The coverage the GPU file relies on, by the model alone."""
    reached = set()
    for _, _, _, log in logs.values():
        for r in log:
            reached |= r["reached"]
    assert [n for n in S.REQUIRED if n not in reached] == [], sorted(reached)
    assert set(S.UNREACHABLE) == set(S.EVENTS + S.BRANCHES) - set(S.REQUIRED)


# ------------------------------------------------------------------------------ layout constants
def test_seg_constants_mirror_the_header():
    from chocosgd_amd import _lib
    src = open(os.path.join(ROOT, "include", "choco_codec.h")).read()
    defs = dict(re.findall(r"^#define CHOCO_(SEG_[A-Z0-9_]+) (\d+)\s*$", src, re.M))
    assert len(defs) == 13 and "SEG_WIN_TRUST" in defs and "SEG_SHADOW_OFFSET" in defs
    for name, value in defs.items():
        assert getattr(_lib, name) == int(value), name
    assert {n for n in dir(_lib) if n.startswith("SEG_")} == set(defs)
    words = [_lib.SEG_WIN_LO, _lib.SEG_WIN_SH, _lib.SEG_WIN_VALID, 12, _lib.SEG_WIN_T_PREV, _lib.SEG_WIN_D_PREV,
             _lib.SEG_WIN_CAND, _lib.SEG_WIN_TRUST]
    assert words == [4 * i for i in range(8)] and len(S.WIN_WORDS) * 4 == _lib.SEG_WIN_STRIDE


def test_diag_layout_and_host_state_are_host_code():
    """choco_topk_segmented_diag_layout against the layout written out by hand once (here and
    nowhere else), and the host-state query on a workspace no call was made on: zeros."""
    from chocosgd_amd import _lib
    lib = _lib.load()

    def align(v):
        return (v + 255) // 256 * 256

    for lens in (S.SMALL, S.EDGES):
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        p_off, keep = _lib.i64_array(offs.tolist())
        plen = lib.choco_topk_segmented_plan_len(p_off, len(lens))
        plan = (ctypes.c_int64 * plen)()
        pp = ctypes.cast(plan, ctypes.POINTER(ctypes.c_int64))
        assert lib.choco_topk_segmented_plan(p_off, len(lens), 0.99, pp) > 0
        nseg, ntile = len(lens), sum((m + 16383) // 16384 for m in lens)
        win, info = ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert lib.choco_topk_segmented_diag_layout(pp, nseg, ctypes.byref(win), ctypes.byref(info)) == 0
        o_info = 256 + 2 * align(nseg * 2048 * 4) + align(nseg * 512 * 4)
        o_win = o_info + align(nseg * 32) + align(ntile * 4) + align(ntile * 8) + 2 * align(ntile * 16384 * 4)
        assert (info.value, win.value) == (o_info, o_win)
        assert win.value + nseg * _lib.SEG_WIN_STRIDE <= lib.choco_topk_segmented_workspace_size(pp, nseg)
        buf = ctypes.create_string_buffer(64)
        out = (ctypes.c_uint64 * 8)(*([7] * 8))
        assert lib.choco_topk_segmented_host_state(ctypes.cast(buf, ctypes.c_void_p), pp, nseg, out) == 0
        assert list(out) == [0] * 8
        assert lib.choco_topk_segmented_host_state(None, pp, nseg, out) != 0
