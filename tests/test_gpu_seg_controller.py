"""GPU: the segmented top-k warm path (csrc/topk_seg.hip: the per-segment windows, the warm
modes, the cold calls' shadow checks and the host's warm / cold choice) held to the plain
model of tests/_seg_controller.py after EVERY call, synchronised: warm or cold, every word of
the host state, the miss counter, the shadow counter, all eight words of every segment's
window and the info words of the window used, as exact integers.  The outputs are exact on
every path, so only this state shows whether the drift, the trust streak, the three window
sources, the backoff and the shadow exit still do what they say.
Run on an MI355X with `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import _seg_controller as S
from conftest import same_bits
from oracle import choco_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = S.gpu_cases()   # the inputs, shared with tests/test_seg_controller_host.py

# the events, window branches and warm modes the sequences of this file went through, the
# device agreeing with the model on every word of the call
REACHED = set()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def run_sequence(lens, ratio, calls, warm=True):
    """Drive `calls` (dicts of tests/_seg_controller._call: x, xhat, mem / gamma for the fused
    consensus step, and the delta d) through codec.topk_segmented on a fresh SegmentPlan and
    hold every call to the model.  Returns the model's records."""
    from chocosgd_amd import _lib as L, codec
    log = S.simulate(lens, ratio, calls, warm)
    plan = codec.SegmentPlan(lens, ratio, torch.device(DEV))
    multi = [s for s, _, _ in S.multi_segments(lens)]
    assert codec.seg_host_state(plan) == dict.fromkeys(codec.SEG_HOST_WORDS, 0)
    oracle, on_dev = {}, {}
    for c, (call, want) in enumerate(zip(calls, log)):
        at = f"call {c} ({'warm' if want['warm'] else 'cold'}, {want['events']})"
        fused = call["mem"] is not None
        hist_0, miss_0 = codec.launch_count("topk_seg_hist"), codec.topk_fallback_count(plan=plan)
        # ---- 1. the call, exact against the oracle
        if id(call) not in on_dev or fused:
            on_dev[id(call)] = (dev(call["x"]), dev(call["xhat"]) if call["xhat"] is not None else None)
        x, xh = on_dev[id(call)]
        if fused:
            vals, idx = codec.topk_segmented(x, plan, xhat=xh, gossip=(dev(call["mem"]), call["gamma"]))
            assert same_bits(host(x), O.gossip_step(call["x"], call["mem"], call["xhat"], call["gamma"])), at
        else:
            vals, idx = codec.topk_segmented(x, plan, xhat=xh)
        torch.cuda.synchronize()
        if id(call) not in oracle:
            oracle[id(call)] = O.topk_segmented(call["d"], lens, ratio)
        ov, oi, _ = oracle[id(call)]
        assert np.array_equal(host(idx).astype(np.int64), oi), at
        assert same_bits(host(vals), ov), at
        # ---- 2. warm or cold
        assert (codec.launch_count("topk_seg_hist") - hist_0 == 0) == want["warm"], at
        # ---- 3. the host state, every word
        got_host = codec.seg_host_state(plan)
        assert got_host == want["host"], (at, got_host, want["host"])
        # ---- 4. the miss counter: segments whose window missed (an overflow is not one)
        assert codec.topk_fallback_count(plan=plan) - miss_0 == want["misses"], at
        assert want["warm"] or want["misses"] == 0, at
        # ---- 5. the shadow counter: (misses << 32 | checks), moved by cold calls only
        assert codec.seg_shadow(plan) == (want["shadow"] >> 32, want["shadow"] & S.U32), at
        # ---- 6. every multi-tile segment's window, all eight words
        wins = codec.seg_windows(plan)
        for s in multi:
            r = want["segs"][s]
            assert tuple(int(v) for v in wins[s]) == r["win"], (at, s, r["source"], sorted(r["branches"]),
                                                              tuple(int(v) for v in wins[s]), r["win"])
        for s in set(range(len(lens))) - set(multi):
            assert not wins[s].any(), (at, s)       # single-tile segments carry no window
        # ---- 7. after a warm call: the window it used is the one the previous call prepared
        if want["warm"]:
            info = codec.seg_info(plan)
            for s in multi:
                r = want["segs"][s]
                got = tuple(int(info[s, i]) for i in (L.SEG_INFO_LO, L.SEG_INFO_SH, 3, 4, L.SEG_INFO_MODE))
                assert got == r["info"], (at, s, got, r["info"])
                assert got[:2] == (r["found"][0], min(r["found"][1], S.K_WIN_SH_MAX)), (at, s)
        # ---- 8. the status word
        assert codec.topk_workspace_word(L.TOPK_STATUS_OFFSET, plan=plan) == 0, at
        REACHED.update(want["reached"])
    codec.check_topk_status(wait=True)
    return log


def _run(name):
    lens, ratio, warm, make = CASES[name]
    return run_sequence(lens, ratio, make(), warm=warm)


def _dev_windows(log, word):
    return [{s: v["win"][S.WIN_WORDS.index(word)] for s, v in r["segs"].items()} for r in log]


# ------------------------------------------------------------------------------ stationary
@pytest.mark.parametrize("name", ["stationary-small", "stationary-edges-0.99"])
def test_stationary(name):
    """12 calls of fresh normal deltas: warm from call 1, no miss, every window from the
    window's own bins, no trust streak."""
    log = _run(name)
    assert [r["warm"] for r in log] == [False] + [True] * 11
    assert all(r["misses"] == 0 for r in log)
    assert all(v["source"] == "select" for r in log[1:] for v in r["segs"].values())
    assert all(t <= 1 for w in _dev_windows(log, "trust") for t in w.values())


@pytest.mark.parametrize("ratio", [0.9, 0.999])
def test_stationary_other_ratios(ratio):
    """The same at k = 10 % and 0.1 %: delta dominated by 0.03 k, then by + 8 (at 0.99 by
    4 sqrt(k)).  At these the small segments' k-th keys leave their windows now and then; the
    model says when."""
    _run(f"stationary-edges-{ratio}")


# ------------------------------------------------------------------------------ drift
@pytest.mark.parametrize("up", [False, True], ids=["down", "up"])
def test_steady_drift(up):
    """One buffer scaled by DRIFT_G^c (or its inverse), ~300 keys per call: the streak reaches
    kDriftTrust at call 4 and from then on the drift is applied with its sign (both window
    edges: run_sequence's window equality)."""
    log = _run("drift-up" if up else "drift-down")
    tag = "drift_pos" if up else "drift_neg"
    for s in log[0]["segs"]:
        assert [r["segs"][s]["win"][7] for r in log] == [0, 0, 0, 1, 2, 3, 4, 5]
        assert all(tag in r["segs"][s]["branches"] for r in log[4:])
        assert not any(r["segs"][s]["branches"] & {"drift_pos", "drift_neg"} for r in log[:4])


def test_long_drift_saturates_the_streak():
    log = _run("drift-long")
    assert all(v["win"][7] == S.K_TRUST_MAX for v in log[-1]["segs"].values())


def test_drift_that_reverses():
    """Six calls up, four down: the streak resets and no drift is applied on the reversal."""
    log = _run("drift-reverses")
    for v in log[6]["segs"].values():
        assert "trust_reset" in v["branches"] and not v["branches"] & {"drift_pos", "drift_neg"}
        assert v["win"][6] == 0 and v["win"][7] == 0


# ------------------------------------------------------------------------------ jump and return
def test_jump_misses_far_apart_never_go_cold():
    """x 100 at call 3 (every window missed-high: the select over the candidate lists), held
    35 calls, x 1e-3 (missed-low: over the segment): two isolated misses, every call warm."""
    log = _run("jump-isolated")
    assert [r["warm"] for r in log] == [False] + [True] * 40
    assert [c for c, r in enumerate(log) if r["misses"]] == [3, 38]


def test_jump_misses_close_start_a_run_that_one_clean_call_ends():
    log = _run("jump-recurring")
    assert "recurring_miss_starts_run" in log[7]["events"] and not log[7]["warm"]
    assert "shadow_exit" in log[8]["events"] and log[8]["warm"]


@pytest.mark.parametrize("kind", ["xhat", "gossip"])
def test_jump_with_xhat_and_the_fused_step(kind):
    """The same controller on the keys of x_new - x_hat (formed in fp32 as the device does)."""
    log = _run(f"jump-{kind}")
    assert "recurring_miss_starts_run" in log[7]["events"] and "shadow_exit" in log[8]["events"]


@pytest.mark.parametrize("kind", ["xhat", "gossip"])
def test_stationary_with_xhat_and_the_fused_step(kind):
    log = _run(f"stationary-{kind}")
    assert [r["warm"] for r in log] == [False] + [True] * 5 and all(r["misses"] == 0 for r in log)


# ------------------------------------------------------------------------------ ties, wide, all
def test_ties_and_bin_list_overflow():
    """Values on a 1/8 grid (the kept-key lists take {key, count}), then more than kTileList
    distinct keys in the k-th key's bin of one tile: selected exactly, not counted as a miss,
    the next window from the window's own bins."""
    log = _run("ties")
    assert all(v["overflow"] for v in log[5]["segs"].values()) and log[5]["misses"] == 0


def test_count_levels_further_apart_than_any_window():
    """The count levels k +- delta 12 binades apart: the window is T's whole coarse bin (the
    centring on T behind it is unreachable, tests/_seg_controller.py UNREACHABLE)."""
    log = _run("too-wide")
    for r in log[0]["segs"].values():
        assert (r["win"][0], r["win"][1]) == ((r["T"] >> 20) << 20, S.K_WIN_SH_MAX)


def test_take_all():
    """ratio 0.0 on a 2-tile segment: the warm calls write SegWin{0, kWinShMax, 1, 0, ...}."""
    log = _run("take-all")
    assert all(v["win"] == S.TAKE_ALL_WIN for r in log[1:] for v in r["segs"].values())


# ------------------------------------------------------------------------------ the cold run
def test_cold_run_runs_out_doubles_and_exits():
    """a / 2a alternating: miss, miss, 64 cold calls whose shadow checks all miss (the run runs
    out), a warm isolated miss, a warm recurring miss (backoff 128), then stationary deltas:
    the first clean cold call ends the run and the backoff is 64 again."""
    log = _run("cold-run")
    assert "cold_run_ran_out" in log[66]["events"]
    assert (log[69]["host"]["backoff"], log[69]["host"]["cold_left"]) == (128, 127)
    assert log[70]["events"] == ("shadow_exit", "backoff_halved", "warm") and log[70]["host"]["backoff"] == 64


def test_warm_start_off():
    """Every call cold; the windows and the shadow counter still advance as the model says."""
    from chocosgd_amd import codec
    lib = codec.lib()
    lib.choco_topk_set_warm_start(0)
    try:
        log = _run("warm-off")
    finally:
        lib.choco_topk_set_warm_start(1)
    assert not any(r["warm"] for r in log) and log[-1]["shadow"] & S.U32 == 5 * log[-1]["nmulti"]


# ------------------------------------------------------------------------------ unsynchronised
def test_unsynchronised_calls_keep_the_invariants():
    """40 calls of the jump pattern launched back to back (the host runs ahead of the device:
    the call at which a miss flag is seen is not deterministic): every output exact, the host
    state within its invariants, the status word 0."""
    from chocosgd_amd import _lib as L, codec
    lens, ratio = S.EDGES, 0.99
    base = S.normal(sum(lens), 1000)
    arrays = {s: base * np.float32(s) for s in (1.0, S.JUMP_UP, S.JUMP_DOWN)}
    oracle = {s: O.topk_segmented(a, lens, ratio) for s, a in arrays.items()}
    xs = {s: dev(a) for s, a in arrays.items()}
    scales = (S.JUMP_RECURRING * 4)[:40]
    plan = codec.SegmentPlan(lens, ratio, torch.device(DEV))
    outs = [(torch.empty(plan.k_total, device=DEV), torch.empty(plan.k_total, dtype=torch.int32, device=DEV))
            for _ in scales]
    torch.cuda.synchronize()
    for s, out in zip(scales, outs):
        codec.topk_segmented(xs[s], plan, out=out)
    torch.cuda.synchronize()
    for c, (s, (vals, idx)) in enumerate(zip(scales, outs)):
        ov, oi, _ = oracle[s]
        assert np.array_equal(host(idx).astype(np.int64), oi), c
        assert same_bits(host(vals), ov), c
    st = codec.seg_host_state(plan)
    assert st["calls"] == 40
    assert st["cold_left"] <= st["backoff"] <= S.K_COLD_MAX
    assert st["backoff"] == 0 or st["backoff"] in [S.K_COLD_MIN << i for i in range(7)]
    assert codec.topk_workspace_word(L.TOPK_STATUS_OFFSET, plan=plan) == 0
    codec.check_topk_status(wait=True)


# ------------------------------------------------------------------------------ reached branches
def test_every_named_branch_was_reached():
    """Needs the whole file to have run: every host event, window branch and warm mode of
    S.REQUIRED occurred in some sequence above with the device agreeing on every word."""
    missing = [b for b in S.REQUIRED if b not in REACHED]
    assert not missing, (missing, sorted(REACHED))
