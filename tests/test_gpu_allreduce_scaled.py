"""The all-reduce SGD step with a global-norm clip and dynamic loss scaling on the device: the
scaled pack (csrc/params.hip, param_pack_scaled_kernel), the norm launch that leaves the
loss-scale state alone, the flat-gradient kernels that skip on the all-reduced flag
(csrc/sgd.hip), loss_scale_update_kernel (csrc/gradnorm.hip), and
utils.allreduce_sgd_step(clip_norm=, loss_scale=).

Everything is compared bit for bit against the numpy model (tests/_allreduce_scaled_oracle.py),
the torch loop, torch's own _amp_* ops and the reference's recorded steps.  Whole storages are
compared, so that every byte a launch does not own is checked together with the ones it does."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden, same_bits
import _allreduce_oracle as AO
import _allreduce_scaled_oracle as ASO
import _gclip_oracle as GO
import _lscale_oracle as LO
import _master_oracle as MA
import _mp_allreduce_scaled_worker as W
import _sgd_oracle as SO
import test_allreduce_scaled_host as H  # Run: one rank beside its numpy model; the fixture replay
import test_gpu_param_sgd as PS  # the guarded layouts and value lists of the SGD kernel's tests

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES, NAMES, SENTINEL = PS.DTYPES, PS.NAMES, PS.SENTINEL
F32 = torch.float32
host = MA.host
LAYOUT = [40, 8192 + 24, 7, 300, 4097]
NEW = ("param_pack_scaled_kernel", "param_gradnorm_scaled_local_total_kernel", "loss_scale_update_kernel",
       "param_sgd_flatgrad_scaled_kernel", "param_sgd_master_flatgrad_scaled_kernel")
OLD = ("param_pack_kernel", "param_sgd_flatgrad_kernel", "param_sgd_master_flatgrad_kernel",
       "param_gradnorm_total_kernel", "param_gradnorm_scaled_total_kernel", "param_sqnorm_kernel",
       "param_unpack_kernel", "param_sgd_kernel", "param_sgd_master_kernel")


def _counts(names=NEW + OLD):
    from chocosgd_amd import codec
    return np.array([codec.launch_count(nm) for nm in names])


def _delta(c0, names=NEW + OLD):
    return dict(zip(names, (_counts(names) - c0).tolist()))


def _guarded(values, shift, extra=8):
    """An fp32 view at element `shift` of a sentinel-filled allocation."""
    n = int(np.size(values))
    big = torch.full((n + shift + extra,), SENTINEL, device=DEV)
    if n:
        big[shift:shift + n] = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(DEV)
    return big, big[shift:shift + n]


def _check_guarded(big, shift, values, what):
    want = torch.full_like(big, SENTINEL)
    n = int(np.size(values))
    if n:
        want[shift:shift + n] = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(DEV)
    assert same_bits(host(big), host(want)), what


# ----------------------------------------------------------------------------- the scaled pack
def run_pack(lens, mode, coef=0.37, round=True, found=None, lead=0, gap=8, own=False, flat_shift=4, seed=3000):
    """One ParamSgdPlan.pack_grads(coef=, found=, round=) on guarded storages against the model;
    returns the launches.  found: None, or the value gradnorm_scaled's third float holds."""
    from chocosgd_amd import codec
    k, n = len(lens), sum(lens)
    dts = PS._dtypes(mode, k)
    G = PS.Guarded(lens, dts, seed, -4, 0, lead, gap, own)  # special values among the gradients
    plan = codec.ParamSgdPlan(G.views)
    for i, v in enumerate(G.views):
        plan.grad_ptrs[i] = v.data_ptr()
    out = [123.0, coef] if found is None else [123.0, coef, found, 64.0]
    bigc, cview = _guarded(np.array(out, np.float32), 3)
    slots = n + (0 if found is None else 1)
    bigf, flat = _guarded(np.full(slots, SENTINEL, np.float32), flat_shift)
    want = [ASO.pack(host(v), np.float32(coef), NAMES[dt], round=round) for v, dt in zip(G.views, dts)]
    if found is not None:
        want.append(np.array([0.0 if found == 0 else 1.0], np.float32))
    c0 = _counts()
    plan.pack_grads(flat, coef=cview, found=None if found is None else cview, round=round)
    d = _delta(c0)
    G.check([None] * k, "the gradients (or their guards) were written")
    _check_guarded(bigc, 3, np.array(out, np.float32), "the coefficient tensor was written")
    _check_guarded(bigf, flat_shift, np.concatenate(want) if want else np.zeros(0, np.float32),
                   "flat, the flag slot or the guards: without `found` element n keeps its sentinel")
    assert d.pop("param_pack_scaled_kernel") == codec.params_launches(k) and not any(d.values()), d
    return codec.params_launches(k)


@pytest.mark.parametrize("round", [True, False], ids=["round", "fp32"])
@pytest.mark.parametrize("coef", [1.0, 0.37, 2.0 ** -4])
@pytest.mark.parametrize("mode", PS.MODES)
def test_pack_views_at_element_alignment(mode, coef, round):
    """Views into one allocation at gaps 1, 2 and 3 behind one leading element: every residue
    of the element offset; inf, NaN, +-0 and subnormal gradients keep their kind."""
    for gap in (1, 2, 3):
        run_pack(PS.BASE, mode, coef, round, found=0.0 if gap == 2 else None, lead=1, gap=gap)


@pytest.mark.parametrize("round", [True, False], ids=["round", "fp32"])
@pytest.mark.parametrize("mode", PS.MODES)
def test_pack_aligned_layout_and_one_side_off_the_grid(mode, round):
    """Every side on the 16-byte grid (the vector path), then the gradients, then flat moved by
    one element: the whole tensor moves element by element and no neighbouring byte changes."""
    lens = [40, 8192 + 24, 8, 304]
    run_pack(lens, mode, 0.37, round, found=1.0, own=True)
    run_pack(lens, mode, 0.37, round, found=1.0, own=True, lead=1)
    run_pack(lens, mode, 0.37, round, found=0.0, own=True, flat_shift=5)


@pytest.mark.parametrize("mode", PS.MODES)
def test_pack_a_tensor_across_several_tiles_and_zero_lengths(mode):
    run_pack([3 * 8192 + 5], mode, own=True, found=2.0)
    run_pack([100, 3 * 8192 + 77, 50], mode, gap=8)
    run_pack([0, 5, 0, 0, 4100, 0], mode, found=0.0)
    run_pack([0, 304, 0, 8200, 40], mode, own=True, round=False)


@pytest.mark.parametrize("found", [None, 0.0, 1.0, float("nan")])
@pytest.mark.parametrize("count", [191, 192, 193])
def test_pack_chunk_boundaries_and_the_flag_written_once(count, found):
    """192 tensors per launch: at 193 the layout takes two launches and the first alone
    carries the flag; the slot is exactly 0.0 or 1.0 whatever nonzero value `found` holds."""
    lens = [1 + i % 13 for i in range(count)]
    assert run_pack(lens, "mixed", found=found, gap=1, lead=1) == -(-count // 192)


@pytest.mark.parametrize("rem", range(8))
def test_pack_flag_at_every_lane_position_behind_a_group(rem):
    """n % 8 in 0..7 with every side on the 16-byte grid: flat[n] sits on each position behind
    the last 16-byte group; without `found` that element keeps its sentinel."""
    for mode in ("fp32", "fp16"):
        run_pack([8192 + 16 + rem], mode, found=1.0, own=True)
        run_pack([16, 8 + rem], mode, found=None, own=True, round=False)


# ----------------------------------------------------------------------------- the norm launch without the state update
@pytest.mark.parametrize("max_norm", [None, 0.4])
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_gradnorm_scaled_local_gives_the_same_out_and_leaves_the_state(mode, max_norm):
    from chocosgd_amd import codec, utils
    dts = PS._dtypes(mode, len(LAYOUT))
    rng = np.random.RandomState(5)
    for bad in (False, True):
        vals = [SO.to_grid((rng.standard_normal(m) * 3.0).astype(np.float32), mode) for m in LAYOUT]
        if bad:
            vals[3][17] = np.inf
        grads = [torch.from_numpy(v).to(DEV).to(dt) for v, dt in zip(vals, dts)]
        plan = codec.ParamSgdPlan(grads)
        for i, g in enumerate(grads):
            plan.grad_ptrs[i] = g.data_ptr()
        scaler = utils.LossScaler(DEV, init_scale=100.0, growth_interval=6)
        scaler._growth_tracker.fill_(5)
        c0 = _counts()
        local = host(plan.gradnorm_scaled(scaler, max_norm, update_state=False))
        d = _delta(c0)
        assert scaler.get_scale() == 100.0 and int(scaler._growth_tracker) == 5, "the state moved"
        assert d["param_gradnorm_scaled_local_total_kernel"] == 1 and d["param_gradnorm_scaled_total_kernel"] == 0
        assert sum(d.values()) == codec.params_gradnorm_launches(len(LAYOUT))
        both = host(plan.gradnorm_scaled(scaler, max_norm))
        assert same_bits(local, both) and local[2] == float(bad) and local[3] == 100.0
        assert scaler.get_scale() == (50.0 if bad else 200.0) and int(scaler._growth_tracker) == 0
        if not bad:
            assert H.near_total(vals, 100.0, mode, local[0])
            assert same_bits(local, LO.out(local[0], max_norm, 100.0, False, mode))


# ----------------------------------------------------------------------------- the flat-gradient kernels with the flag slot
def run_flatgrad(lens, mode, master, flag, lead=(0, 0, 0), gap=8, own=False, gsum_shift=4, seed=7000):
    """codec.params_sgd_flatgrad(found_slot=True) on guarded storages: with gsum[n] == 0 against
    the unscaled entry point on a twin, bit for bit; otherwise nothing at all may change."""
    from chocosgd_amd import codec
    k, n = len(lens), sum(lens)
    dts = PS._dtypes(mode, k)
    hps = [PS._varied_hp(i) for i in range(k)]
    firsts = [i % 2 == 0 and hps[i][2] != 0 for i in range(k)]
    cols = [[h[j] for h in hps] for j in range(5)]
    s_all = np.concatenate([PS._values(m, seed + 30000 + i, -4, 0) for i, m in enumerate(lens)] +
                           [np.array([flag], np.float32)])
    m0 = np.concatenate([PS._values(m, seed + 20000 + i, -3, 1) for i, m in enumerate(lens)])
    sides = []
    for scaled in (True, False):
        P = PS.Guarded(lens, dts, seed, -3, 1, lead[0], gap, own)
        G = PS.Guarded(lens, dts, seed + 5000, -4, 0, lead[1], gap, own)
        B = PS.Guarded(lens, [F32] * k if master else dts, seed + 9000, -4, 0, lead[2], gap, own)
        bigs, gsum = _guarded(s_all if scaled else s_all[:n], gsum_shift)
        bigm, mview = _guarded(m0, 4)
        c0 = _counts()
        codec.params_sgd_flatgrad(P.views, G.views, [b if hps[i][2] != 0 else None for i, b in enumerate(B.views)],
                                  gsum, 3.0, *cols, firsts, master=mview if master else None, found_slot=scaled)
        d = _delta(c0)
        name = "param_sgd_" + ("master_" if master else "") + "flatgrad" + ("_scaled" if scaled else "") + "_kernel"
        assert d.pop(name) == codec.params_sgd_flatgrad_launches(k) and not any(d.values()), d
        _check_guarded(bigs, gsum_shift, s_all if scaled else s_all[:n], "gsum was written")
        sides.append((P, G, B, bigm))
    (P, G, B, bigm), twin = sides
    if flag == 0:
        for a, b, what in zip((P, G, B), twin[:3], ("params", "grads", "momentum buffers")):
            assert all(same_bits(host(x), host(y)) for x, y in zip(a.stores, b.stores)), what
        assert same_bits(host(bigm), host(twin[3])), "master"
        assert not all(same_bits(host(x), host(y)) for x, y in zip(P.stores, P.before)), "nothing moved"
    else:
        P.check([None] * k, "a skipped step wrote a parameter (or a guard)")
        G.check([None] * k, "a skipped step wrote a gradient (or a guard)")
        B.check([None] * k, "a skipped step wrote a momentum buffer (or a guard)")
        _check_guarded(bigm, 4, m0, "a skipped step wrote the master copy")


@pytest.mark.parametrize("flag", [0.0, 1.0, 2.0, float("nan")])
@pytest.mark.parametrize("master", [False, True], ids=["plain", "master"])
@pytest.mark.parametrize("mode", PS.MODES)
def test_flatgrad_scaled_views_and_aligned_layouts(mode, master, flag):
    run_flatgrad(PS.BASE, mode, master, flag, lead=(1, 1, 1), gap=3)
    run_flatgrad([40, 8192 + 24, 8, 304], mode, master, flag, own=True)
    run_flatgrad([0, 5, 0, 4100, 3 * 8192 + 5], mode, master, flag, gsum_shift=5)


@pytest.mark.parametrize("flag", [0.0, 1.0])
@pytest.mark.parametrize("master", [False, True], ids=["plain", "master"])
@pytest.mark.parametrize("count", [72, 73])
def test_flatgrad_scaled_chunk_boundaries(count, master, flag):
    run_flatgrad([1 + i % 13 for i in range(count)], "mixed", master, flag, gap=1, lead=(1, 1, 1))


# ----------------------------------------------------------------------------- the state update
@pytest.mark.parametrize("tracker", [0, 6, 7])
@pytest.mark.parametrize("flag", [0.0, 1.0, 3.0, float("nan")])
def test_loss_scale_update_against_the_model_and_torch(flag, tracker):
    """found / not found, a tracker at interval - 1 and below it, and a growth that would
    overflow to inf (kept out), against _lscale_oracle.update and torch._amp_update_scale_."""
    from chocosgd_amd import codec, utils
    n = 37
    plan = codec.ParamSgdPlan([torch.zeros(n, device=DEV)])
    for scale, growth in ((1000.0, 2.0), (3.0e38, 2.0), (0.75, 1.5)):
        scaler = utils.LossScaler(DEV, init_scale=scale, growth_factor=growth, backoff_factor=0.25, growth_interval=8)
        scaler._growth_tracker.fill_(tracker)
        scaler.last = torch.tensor([5.0, 6.0, 7.0, scale], device=DEV)
        big, gsum = _guarded(np.concatenate([np.full(n, 2.5, np.float32), [flag]]), 3)
        ts, tt = scaler._scale.clone(), scaler._growth_tracker.clone()
        found = flag != 0
        torch._amp_update_scale_(ts, tt, torch.tensor([float(found)], device=DEV), growth, 0.25, 8)
        c0 = _counts()
        plan.loss_scale_update(scaler, gsum)
        d = _delta(c0)
        assert d.pop("loss_scale_update_kernel") == 1 and not any(d.values()), d
        want_s, want_t = LO.update(np.float32(scale), tracker, found, growth, 0.25, 8)
        assert same_bits(host(scaler._scale), [want_s]) and int(scaler._growth_tracker) == want_t
        assert torch.equal(scaler._scale, ts) and torch.equal(scaler._growth_tracker, tt), "torch's own op"
        assert np.isfinite(host(scaler._scale)[0])
        assert same_bits(host(scaler.last), [5.0, 6.0, float(found), scale]), "last[2] is the common flag, only it"
        _check_guarded(big, 3, np.concatenate([np.full(n, 2.5, np.float32), [flag]]), "gsum was written")


# ----------------------------------------------------------------------------- end to end
class DeviceRun(H.Run):
    """H.Run on device tensors; a clip-only step through the kernels is held to the total the
    norm launch left on the device."""

    def __init__(self, mode, master, kind, entry="step", **kw):
        kw.setdefault("lens", LAYOUT)
        kw.setdefault("hps", [PS._varied_hp(i) for i in range(len(kw["lens"]))])
        super().__init__(mode, master, kind, entry, device=DEV, **kw)
        self.entry = entry

    def clip_total(self, before):
        from chocosgd_amd import utils
        if self.entry == "loop":
            return super().clip_total(before)
        return None if before else float(utils._sgd_plan(self.params)._gn_out[0])


@pytest.mark.parametrize("kind", sorted(H.KINDS))
@pytest.mark.parametrize("master", [False, True], ids=["plain", "master"])
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_step_equals_the_loop_and_the_model(mode, master, kind):
    """Three steps of world 3 through the kernels and through the torch loop, each against the
    numpy model at its own total (equal or adjacent to float32(sqrt(fp64 sum of squares))); the
    loop of a clip-only step is pinned to the kernels' total, and wherever the two totals are
    the same bits so is everything else.  The launches of every step."""
    from chocosgd_amd import codec
    step, loop = DeviceRun(mode, master, kind, "step"), DeviceRun(mode, master, kind, "loop")
    k = len(LAYOUT)
    scaled = H.KINDS[kind][1]
    for j in range(H.STEPS):
        c0 = _counts()
        assert step.step(step.grads(), write_grads=j != 1), j
        d = _delta(c0)
        upd = "param_sgd_" + ("master_" if master else "") + "flatgrad" + ("_scaled" if scaled else "") + "_kernel"
        want = {"param_pack_scaled_kernel": codec.params_launches(k), upd: codec.params_sgd_flatgrad_launches(k),
                "param_sqnorm_kernel": codec.params_gradnorm_launches(k) - 1,
                "param_gradnorm_scaled_local_total_kernel" if scaled else "param_gradnorm_total_kernel": 1}
        if scaled:
            want["loss_scale_update_kernel"] = 1
        assert {nm: c for nm, c in d.items() if c} == want
        assert sum(d.values()) == codec.params_gradnorm_launches(k) + codec.params_launches(k) + int(scaled) + \
            codec.params_sgd_flatgrad_launches(k)
        if not scaled:
            loop.pin = float(step.totals[-1])
        c0 = _counts(NEW)
        assert loop.step(loop.grads(), write_grads=j != 1), j
        assert not any(_delta(c0, NEW).values()), "the loop launched the new kernels"
        if same_bits([step.totals[-1]], [loop.totals[-1]]):
            assert all(same_bits(a, b) for a, b in zip(step.snapshot(), loop.snapshot())), j
    assert not same_bits(H._cat(step.params), H._cat(H._model(mode, 0, LAYOUT, step.mdl.hps, DEV)[0]))


@pytest.mark.parametrize("place", [(0, 3), (1, 8187), (4, 4096)], ids=["first", "middle", "last"])
@pytest.mark.parametrize("master", [False, True], ids=["plain", "master"])
@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_a_step_with_an_inf_is_skipped_and_backs_off(mode, master, place):
    """Taken, skipped, taken: the skipped step leaves parameters, gradients, buffers and master
    as they were (H.Run compares all of them), halves the scale and resets the tracker."""
    run = DeviceRun(mode, master, "both")
    assert run.step(run.grads())
    c0 = _counts()
    assert not run.step(run.grads(bad=(place[0], place[1], np.inf)))
    d = _delta(c0)
    assert d["loss_scale_update_kernel"] == 1, "a skipped step still updates the scale"
    assert run.scaler.get_scale() == H.SCALES[mode] / 2 and int(run.scaler._growth_tracker) == 0
    assert run.step(run.grads())
    assert float(run.scaler.last[3]) == H.SCALES[mode] / 2


@pytest.mark.parametrize("who", ["a peer", "a NaN sum"])
def test_a_peers_overflow_skips_this_rank_too(who):
    run = DeviceRun("fp16", True, "scale")
    assert run.step(run.grads())
    assert not run.step(run.grads(), peer_flag=1.0 if who == "a peer" else np.nan)
    assert run.last_out[2] == 0.0, "this rank's own gradients were finite"
    assert run.step(run.grads())


@pytest.mark.parametrize("master", [False, True], ids=["plain", "master"])
def test_a_skipped_first_step_leaves_no_buffers_and_the_next_takes_first(master):
    """The first step overflows: the created momentum buffers are taken back, no update is
    launched, the scale is still backed off; the next step creates them again (F_FIRST: the
    model's first step, dampening and all)."""
    run = DeviceRun("fp16", master, "both")
    c0 = _counts()
    assert not run.step(run.grads(bad=(1, 5000, np.nan)))
    d = _delta(c0)
    assert d["loss_scale_update_kernel"] == 1
    assert d["param_sgd_flatgrad_scaled_kernel"] == 0 and d["param_sgd_master_flatgrad_scaled_kernel"] == 0
    assert all("momentum_buffer" not in run.state[p] for p in run.params)
    assert run.step(run.grads()) and run.step(run.grads())


def test_fp32_step_equals_torchs_unscale_clip_average_and_update():
    """A power-of-two scale: multiplying by 1 / scale is exact, so the scaled step equals
    _amp_foreach_non_finite_check_and_unscale_, clip_grad_norm_loop at the same total, today's
    allreduce_sgd_step and _amp_update_scale_ on a twin, bit for bit; step 1 overflows."""
    from chocosgd_amd import utils
    hps = [PS._varied_hp(i) for i in range(len(LAYOUT))]
    n = sum(LAYOUT)
    a, ga, names, rng = H._model("fp32", 3, LAYOUT, hps, DEV)
    b, gb, _, _ = H._model("fp32", 3, LAYOUT, hps, DEV)
    sa, sb = collections.defaultdict(dict), collections.defaultdict(dict)
    scaler = utils.LossScaler(DEV, init_scale=4096.0, growth_interval=2)
    scale_b, tracker_b = torch.full((1,), 4096.0, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    for k in range(4):
        raw = [SO.mul32(rng.standard_normal(m).astype(np.float32), host(scale_b)[0]) for m in LAYOUT]
        if k == 1:
            raw[2][3] = -np.inf
        peers = [(0.1 * rng.standard_normal(n)).astype(np.float32) for _ in range(2)]
        for q, r, v in zip(a, b, raw):
            q.grad, r.grad = torch.from_numpy(v.copy()).to(DEV), torch.from_numpy(v.copy()).to(DEV)
        agg = AO.Loopback(3, peers=[[np.concatenate([q, [0.0]]).astype(np.float32) for q in peers]])
        assert utils.allreduce_sgd_step(ga, names, sa, agg, clip_norm=0.4, loss_scale=scaler) == 32 * (n + 1)
        found = torch.zeros(1, device=DEV)
        torch._amp_foreach_non_finite_check_and_unscale_([q.grad for q in b], found, scale_b.double().reciprocal().float())
        if not bool(found):
            utils.clip_grad_norm_loop(b, 0.4, total_norm=scaler.last[0])
            utils.allreduce_sgd_step(gb, names, sb, AO.Loopback(3, peers=[peers]))
        torch._amp_update_scale_(scale_b, tracker_b, found, 2.0, 0.5, 2)
        assert scaler.skipped() == (k == 1)
        assert same_bits(H._cat(a), H._cat(b)), f"params after step {k}"
        if k != 1:
            assert same_bits(H._cat([q.grad for q in a]), H._cat([q.grad for q in b])), f"gradients after step {k}"
        for q, r in zip(a, b):
            assert ("momentum_buffer" in sa[q]) == ("momentum_buffer" in sb[r])
            if "momentum_buffer" in sa[q]:
                assert same_bits(host(sa[q]["momentum_buffer"]), host(sb[r]["momentum_buffer"]))
        assert torch.equal(scaler._scale, scale_b) and torch.equal(scaler._growth_tracker, tracker_b)
    assert scaler.get_scale() == 4096.0  # halved at step 1, doubled after steps 2 and 3


# ----------------------------------------------------------------------------- the reference's recorded steps
@pytest.mark.parametrize("master", [False, True], ids=["plain", "master"])
@pytest.mark.parametrize("name", H.SETS)
def test_fixture_replay(name, master):
    """clip_grad_norm_ then the reference's centralized SGD.step, three steps of world 3, through
    the kernels with the total pinned to what torch returned: bit for bit."""
    from chocosgd_amd import codec, utils
    c0 = _counts()
    agg = H.replay(utils.allreduce_sgd_step, DEV, name, master, "recorded sum")
    d = _delta(c0)
    inputs = golden("allreduce_clip_inputs")
    k = len(inputs["lens"])
    for j in range(H.STEPS):
        c = GO.coef(inputs[f"total0_{j}"], float(inputs["max_norm"]))
        assert same_bits(agg.seen[j], GO.clip(inputs[f"g{j}"], c)), "the packed, clipped gradients"
    upd = "param_sgd_master_flatgrad_kernel" if master else "param_sgd_flatgrad_kernel"
    want = {"param_pack_scaled_kernel": H.STEPS * codec.params_launches(k), "param_gradnorm_total_kernel": H.STEPS,
            upd: H.STEPS * codec.params_sgd_flatgrad_launches(k)}
    if master:
        want["param_pack_kernel"] = codec.params_launches(k)  # MasterWeights packs the parameters once
    assert {nm: c for nm, c in d.items() if c} == want


# ----------------------------------------------------------------------------- launches and syncs
@pytest.mark.parametrize("master", [False, True], ids=["plain", "master"])
def test_launch_counts(master):
    """A scaled step is the norm launches, the pack's, one for the scale and the update's; a
    clip-only step has no scale launch; without the keywords the step is today's, launch for
    launch, and none of the new kernels runs."""
    from chocosgd_amd import codec
    k = 193  # two pack launches, two norm-pass launches, three update launches
    lens = [1 + i % 13 for i in range(k)]
    upd = "param_sgd_master_flatgrad" if master else "param_sgd_flatgrad"
    got = {}
    for kind in ("both", "scale", "clip"):
        run = DeviceRun("fp16", master, kind, lens=lens)
        c0 = _counts()
        assert run.step(run.grads())
        got[kind] = {nm: c for nm, c in _delta(c0).items() if c}
    norm, pack, update = (codec.params_gradnorm_launches(k), codec.params_launches(k),
                          codec.params_sgd_flatgrad_launches(k))
    assert (norm, pack, update) == (3, 2, 3)
    for kind in ("both", "scale"):
        assert got[kind] == {"param_sqnorm_kernel": norm - 1, "param_gradnorm_scaled_local_total_kernel": 1,
                             "param_pack_scaled_kernel": pack, "loss_scale_update_kernel": 1,
                             upd + "_scaled_kernel": update}
    assert got["clip"] == {"param_sqnorm_kernel": norm - 1, "param_gradnorm_total_kernel": 1,
                           "param_pack_scaled_kernel": pack, upd + "_kernel": update}
    from chocosgd_amd import utils
    run = DeviceRun("fp16", master, "clip", lens=lens)
    for p, g in zip(run.params, run.grads()):
        p.grad = torch.from_numpy(g).to(DEV).to(p.dtype)
    c0 = _counts()
    utils.allreduce_sgd_step(run.groups, run.names, run.state, AO.Loopback(3, peers=[[]]), master=run.mw,
                             clip_norm=None, total_norm=None, loss_scale=None)
    assert {nm: c for nm, c in _delta(c0).items() if c} == {"param_pack_kernel": pack, upd + "_kernel": update}


class DevicePeer:
    """An aggregator that adds a device-resident peer buffer: nothing of it touches the host."""

    def __init__(self, peer):
        self.world_size, self.peer = 2.0, peer

    def _agg(self, data, op=None, distributed=True):
        return data.add_(self.peer)


@pytest.mark.parametrize("bad", [False, True], ids=["taken", "skipped"])
def test_no_host_sync_in_steady_state(bad):
    """After the first taken step (which creates the buffers and reads the summed flag), a step
    syncs nothing, taken or skipped: the skip is the device's."""
    from chocosgd_amd import utils
    run = DeviceRun("fp16", True, "both")
    assert run.step(run.grads())
    raw = run.grads(bad=(1, 77, np.inf) if bad else None)
    for p, g in zip(run.params, raw):
        p.grad = torch.from_numpy(g).to(DEV).to(p.dtype)
    peer = torch.zeros(run.n + 1, device=DEV)
    before = run.snapshot()
    probe = torch.ones(1, device=DEV)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            armed = False
        except RuntimeError:
            armed = True
        if armed:
            bits = utils.allreduce_sgd_step(run.groups, run.names, run.state, DevicePeer(peer), master=run.mw,
                                            clip_norm=0.4, loss_scale=run.scaler)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    if not armed:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not catch .item() on this build")
    assert bits == 32 * (run.n + 1) and run.scaler.skipped() == bad
    out = run.mdl.local(raw, 0.4, total=host(run.scaler.last)[0])
    assert run.mdl.apply(ASO.add([run.mdl.flat(raw, out), np.zeros(run.n + 1, np.float32)]), 2.0) == (not bad)
    if bad:
        assert all(same_bits(a, b) for a, b in zip(before, run.snapshot()))
    else:
        assert same_bits(host(run.mw.buffer), run.mdl.cat("cur")) and same_bits(H._cat(run.params), run.mdl.cat("p16"))


# ----------------------------------------------------------------------------- refusals
def test_python_refusals_change_nothing():
    from chocosgd_amd import codec, utils
    run = DeviceRun("bf16", True, "both", lens=[40, 300, 7])
    n = run.n
    for p, g in zip(run.params, run.grads()):
        p.grad = torch.from_numpy(g).to(DEV).to(p.dtype)
    agg = AO.Loopback(3, peers=[[np.zeros(n + 1, np.float32)] * 2] * 8)
    before = run.snapshot()
    c0 = _counts()
    with pytest.raises(RuntimeError, match="total_norm"):
        utils.allreduce_sgd_step(run.groups, run.names, run.state, agg, master=run.mw, clip_norm=0.4, total_norm=1.0,
                                 loss_scale=run.scaler)
    with pytest.raises(RuntimeError, match="clip_norm"):
        utils.allreduce_sgd_step(run.groups, run.names, run.state, agg, master=run.mw, total_norm=1.0)
    with pytest.raises(RuntimeError, match="LossScaler"):
        utils.allreduce_sgd_step(run.groups, run.names, run.state, agg, master=run.mw, loss_scale=1024.0)
    run.state[run.params[1]]["momentum_buffer"] = torch.zeros_like(run.params[1])  # a 16-bit buffer
    with pytest.raises(RuntimeError, match="float32 momentum buffers"):
        utils.allreduce_sgd_step(run.groups, run.names, run.state, agg, master=run.mw, loss_scale=run.scaler)
    del run.state[run.params[1]]["momentum_buffer"]
    # the codec's own entry points
    plan = codec.ParamSgdPlan([p.data for p in run.params])
    for i, p in enumerate(run.params):
        plan.grad_ptrs[i] = p.grad.data_ptr()
    two, four = torch.ones(2, device=DEV), torch.ones(4, device=DEV)
    flat = torch.zeros(n, device=DEV)
    for kw in (dict(coef=two, found=four), dict(found=four), dict(coef=torch.ones(3, device=DEV)),
               dict(coef=two.cpu()), dict(coef=two.double()), dict(coef=two, found=two)):
        with pytest.raises(RuntimeError):  # flat holds n elements: no room for the flag; found without coef; ...
            plan.pack_grads(flat, **kw)
    with pytest.raises(RuntimeError):  # n + 1 elements without found
        plan.pack_grads(torch.zeros(n + 1, device=DEV), coef=two)
    with pytest.raises(RuntimeError):  # gsum of n elements with the flag slot
        plan.run_flatgrad(flat, 3.0, found_slot=True)
    with pytest.raises(RuntimeError):  # gsum of n + 1 elements without it
        plan.run_flatgrad(torch.zeros(n + 1, device=DEV), 3.0)
    with pytest.raises(RuntimeError):  # no `last` to put the flag into
        plan.loss_scale_update(utils.LossScaler(DEV), torch.zeros(n + 1, device=DEV))
    run.scaler.last = four
    with pytest.raises(RuntimeError):  # gsum without the slot
        plan.loss_scale_update(run.scaler, flat)
    run.scaler.last = None
    assert not any(_delta(c0).values()), "a refused call launched something"
    assert agg.calls == 0
    assert run.scaler.get_scale() == H.SCALES["bf16"] and int(run.scaler._growth_tracker) == 0
    assert all(same_bits(a, b) for a, b in zip(before, run.snapshot()))
    assert all("momentum_buffer" not in run.state[p] for p in run.params)


# ----------------------------------------------------------------------------- across processes
@pytest.mark.parametrize("mode,world,kind", [("fp32", 2, "scale"), ("fp32", 3, "scale"), ("fp16", 2, "scale"),
                                             ("fp16", 3, "scale"), ("fp16_master", 2, "scale"),
                                             ("fp16_master", 3, "scale"), ("fp32", 2, "both"),
                                             ("fp16_master", 2, "both")])
def test_allreduce_scaled_step_across_processes(mode, world, kind, tmp_path):
    """utils.allreduce_sgd_step(loss_scale=) on `world` ranks sharing the one GPU, the all-reduce
    over gloo with host staging (tests/_mp_allreduce_scaled_worker.py, a fresh interpreter).
    At step 1 rank 1 alone holds one inf: every rank skips, and every rank's scale and tracker
    stay the same bits.  Unscaled gradients are multiples of 2^-4 in [-2, 2] and the scales powers
    of two: scaled values are exact in fp16 and every partial sum of three ranks is exact in any
    order.  With a clip (a non-dyadic coefficient per rank) the world is 2: a sum of two does not
    depend on the order.  Steps 0 and 2 against the model, step 2 with the backed-off scale."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_mp_allreduce_scaled_worker.py"), mode, str(world),
                        kind, str(tmp_path)], capture_output=True, text=True, timeout=W.TIMEOUT * (W.STEPS + 3))
    assert r.returncode == 0, r.stderr[-4000:]
    got = [dict(np.load(tmp_path / f"rank{q}.npz")) for q in range(world)]
    dtype, master = mode.split("_")[0], mode.endswith("_master")
    clip = W.CLIP if kind == "both" else None
    k = len(W.LENS)
    mdl = ASO.Model(W.params0(), [dtype] * k, [W.HP[i % 3] for i in range(k)], master, scale=W.SCALE,
                    interval=W.INTERVAL)
    for step in range(W.STEPS):
        scale = float(mdl.scale)
        assert scale == (W.SCALE if step < 2 else W.SCALE / 2)
        flats = []
        for q in range(world):
            raw = W.grads_of(q, step, scale)
            last = got[q][f"last{step}"]
            assert last[3] == scale and last[2] == float(step == 1), (q, step)
            if step != 1 or q != 1:
                assert H.near_total(raw, scale, ASO.coef_dtype([dtype], master), last[0]), (q, step)
            flats.append(mdl.flat(raw, mdl.local(raw, clip, total=last[0])))
            if clip is None and (step != 1 or q != 1):
                unscaled = np.concatenate(W.grads_of(q, step, 1.0))
                assert same_bits(flats[-1][:-1], unscaled), "the pack unscales exactly"
        before = [mdl.cat("p16"), mdl.cat("bufs"), mdl.cat("cur")]
        taken = mdl.apply(ASO.add(flats), float(world))
        assert taken == (step != 1)
        for q in range(world):
            assert same_bits(got[q][f"p{step}"], mdl.cat("p16")), (q, step)
            assert same_bits(got[q][f"buf{step}"], mdl.cat("bufs")), (q, step)
            if taken:
                assert same_bits(got[q][f"g{step}"], mdl.cat("g16")), (q, step)
            else:
                assert same_bits(got[q][f"g{step}"], np.concatenate(W.grads_of(q, step, scale))), "p.grad was written"
                assert same_bits(got[q][f"p{step}"], before[0]) and same_bits(got[q][f"buf{step}"], before[1])
            if master:
                assert same_bits(got[q][f"m{step}"], mdl.cat("cur")), (q, step)
            assert same_bits(got[q][f"scale{step}"], [mdl.scale]) and int(got[q][f"tracker{step}"][0]) == mdl.tracker
            for key in ("p", "buf", "scale", "tracker") + (("m",) if master else ()):
                assert same_bits(got[q][f"{key}{step}"], got[0][f"{key}{step}"]), (q, key, step)
