"""The all-reduce SGD step with clip_norm / loss_scale, host side (no GPU):
utils.allreduce_sgd_step_loop on CPU tensors (utils.allreduce_sgd_step takes it for CPU tensors
as well) against the numpy model (tests/_allreduce_scaled_oracle.py), bit for bit; the skipped
step; the growth of the scale; the refusal of a pinned total with loss_scale; the reference's
own recorded clip-then-centralized-step fixtures (tests/golden/allreduce_clip_*.npz); and the
argument checks of the new entry points, made before any HIP call."""
import collections
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden, same_bits
import _allreduce_oracle as AO
import _allreduce_scaled_oracle as ASO
import _gclip_oracle as GO
import _lscale_oracle as LO
import _master_oracle as MA
import _sgd_oracle as SO

LENS = [1, 2, 3, 7, 8, 9, 31, 33, 300]
N = sum(LENS)
STEPS = 3
HP = (0.01, 1e-4, 0.9, 0.1, False)
SCALES = {"fp32": 1000.0, "bf16": 1000.0, "fp16": 100.0}  # not powers of two: 1 / scale is rounded
KINDS = {"clip": (0.4, False), "scale": (None, True), "both": (0.4, True)}
host = MA.host


def _model(mode, seed=0, lens=LENS, hps=HP, device="cpu"):
    rng = np.random.RandomState(seed)
    dt = MA.DTYPES[mode]
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(m).astype(np.float32)).to(device).to(dt))
              for m in lens]
    groups, names = AO.groups_of(params, hps)
    return params, groups, names, rng


def near_total(raw, scale, cd, got):
    """Whether `got` is the model's total from float32(sqrt(fp64 sum of squares)) or from one of
    its two fp32 neighbours: the order of the fp64 additions is the implementation's own."""
    root = np.array([GO.total64(raw)]).astype(np.float32)[0]
    inv = np.float32(1.0) if scale is None else LO.inv(scale)
    with np.errstate(all="ignore"):
        cands = [root, np.nextafter(root, np.float32(np.inf)), np.nextafter(root, np.float32(-np.inf))]
        return any(same_bits([got], SO.to_grid(SO.mul32(np.array([x], np.float32), inv), cd)) for x in cands)


def _cat(tensors):
    return np.concatenate([host(t).reshape(-1) for t in tensors])


class Run:
    """One rank of a world of 3 on CPU tensors beside its numpy model."""

    def __init__(self, mode, master, kind, entry="loop", interval=2000, seed=0, lens=LENS, hps=HP, device="cpu",
                 scale=None):
        from chocosgd_amd import utils
        self.mode, self.master, self.lens, self.n, self.device = mode, master, list(lens), sum(lens), device
        self.clip, scaled = KINDS[kind]
        scale = SCALES[mode] if scale is None else scale
        self.params, self.groups, self.names, self.rng = _model(mode, seed, lens, hps, device)
        self.mw = utils.MasterWeights(self.groups, self.names) if master else None
        self.state = collections.defaultdict(dict)
        self.scaler = utils.LossScaler(device, init_scale=scale, growth_interval=interval) if scaled else None
        self.mdl = ASO.Model([host(p) for p in self.params], [mode] * len(lens),
                             [hps] * len(lens) if isinstance(hps, tuple) else hps, master,
                             scale=scale if scaled else None, interval=interval)
        self.fn = utils.allreduce_sgd_step_loop if entry == "loop" else utils.allreduce_sgd_step
        self.cd = ASO.coef_dtype([mode], master)
        self.totals, self.pin = [], None

    def clip_total(self, before):
        """The total a clip-only step runs with: this step's own (the torch ops', computed in
        front of it).  The device test reads the kernels' instead."""
        from chocosgd_amd import utils
        if not before:
            return None
        cd = torch.float32 if self.master else MA.DTYPES[self.mode]
        return float(utils._total_norm([p.grad for p in self.params], None, cd))

    def grads(self, bad=None):
        """Gradients of about 0.1 (times the loss scale), on the dtype's grid."""
        scale = 1.0 if self.scaler is None else float(self.mdl.scale)
        raw = [SO.to_grid(SO.mul32((0.1 * self.rng.standard_normal(m)).astype(np.float32), scale), self.mode)
               for m in self.lens]
        if bad is not None:
            raw[bad[0]][bad[1]] = bad[2]
        return raw

    def step(self, raw, peer_flag=0.0, write_grads=True):
        """One step; returns whether the model took it.  Everything is compared."""
        from chocosgd_amd import utils
        scaled = self.scaler is not None
        for p, g in zip(self.params, raw):
            p.grad = torch.from_numpy(g.copy()).to(self.device).to(p.dtype)
        N = self.n
        peers = [np.concatenate([(0.1 * self.rng.standard_normal(N)).astype(np.float32),
                                 np.array([peer_flag if r == 1 else 0.0], np.float32)[:int(scaled)]]) for r in range(2)]
        agg = AO.Loopback(3, peers=[peers])
        scale0 = None if not scaled else self.scaler.get_scale()
        # the step's own total: the model is held to it, and it to the fp64 root within one fp32 step
        total = None if scaled else self.pin if self.pin is not None else self.clip_total(True)
        before = self.snapshot()
        bits = self.fn(self.groups, self.names, self.state, agg, write_grads=write_grads, master=self.mw,
                       clip_norm=self.clip, loss_scale=self.scaler, total_norm=self.pin)
        assert bits == 32 * (N + int(scaled)), "n_bits counts the buffer sent"
        if scaled:
            total = host(self.scaler.last)[0]
        elif total is None:
            total = self.clip_total(False)
        if self.pin is None and np.isfinite(total):
            assert near_total(raw, scale0, self.cd, total), "the total against float32(sqrt(fp64 sum of squares))"
        self.totals.append(np.float32(total))
        out = self.mdl.local(raw, self.clip, total=total)
        own = self.mdl.flat(raw, out)
        self.last_out, self.last_peers = out, peers
        assert agg.calls == 1 and same_bits(agg.seen[0], own), "the packed gradients (and the flag)"
        taken = self.mdl.apply(ASO.add([own] + peers), 3.0)
        if scaled:
            want_last = out.copy()
            want_last[2] = 0.0 if taken else 1.0
            assert same_bits(host(self.scaler.last), want_last), "last: [total, gc, the GLOBAL flag, scale]"
            assert same_bits(host(self.scaler._scale), [self.mdl.scale]), "the scale"
            assert int(self.scaler._growth_tracker) == self.mdl.tracker, "the tracker"
            assert self.scaler.skipped() == (not taken)
        if not taken:
            assert all(same_bits(a, b) for a, b in zip(before, self.snapshot())), "a skipped step wrote something"
            return False
        assert same_bits(_cat(self.params), self.mdl.cat("p16")), "parameters"
        assert same_bits(_cat([p.grad for p in self.params]),
                         self.mdl.cat("g16") if write_grads else np.concatenate(raw)), "gradients"
        bufs = [self.state[p]["momentum_buffer"] for p in self.params if "momentum_buffer" in self.state[p]]
        assert len(bufs) == sum(b is not None for b in self.mdl.bufs)
        assert all(b.dtype == (torch.float32 if self.master else MA.DTYPES[self.mode]) for b in bufs)
        assert same_bits(_cat(bufs), self.mdl.cat("bufs")), "momentum buffers"
        if self.master:
            assert same_bits(host(self.mw.buffer), self.mdl.cat("cur")), "master"
        return True

    def snapshot(self):
        s = [_cat(self.params), _cat([p.grad for p in self.params])]
        s.append(_cat([self.state[p]["momentum_buffer"] for p in self.params if "momentum_buffer" in self.state[p]])
                 if any("momentum_buffer" in self.state[p] for p in self.params) else np.zeros(0, np.float32))
        s.append(host(self.mw.buffer) if self.master else np.zeros(0, np.float32))
        return s


@pytest.mark.parametrize("entry", ["loop", "step"])
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("master", [False, True], ids=["plain", "master"])
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_cpu_loop_matches_the_model(mode, master, kind, entry):
    run = Run(mode, master, kind, entry)
    for k in range(STEPS):
        assert run.step(run.grads(), write_grads=k != 1), k
    p0 = _model(mode)[0]
    assert len(run.totals) == STEPS
    assert not same_bits(_cat(run.params), _cat(p0)), "the parameters did not move"


@pytest.mark.parametrize("who", ["this rank", "a peer", "a NaN sum"])
@pytest.mark.parametrize("master", [False, True], ids=["plain", "master"])
@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_a_skipped_step_changes_nothing_and_backs_off(mode, master, who):
    """Taken, skipped, taken.  The overflow is this rank's (an inf among its gradients), a
    peer's (its flag slot holds 1.0, this rank's gradients are finite) or a flag sum that is a
    NaN.  The skipped step leaves parameters, gradients, buffers and master as they were, halves
    the scale and resets the tracker; step 2 runs with the backed-off scale."""
    run = Run(mode, master, "both")
    assert run.step(run.grads())
    if who == "this rank":
        assert not run.step(run.grads(bad=(8, 100, np.inf)))
    else:
        assert not run.step(run.grads(), peer_flag=1.0 if who == "a peer" else np.nan)
    assert run.scaler.get_scale() == SCALES[mode] / 2 and int(run.scaler._growth_tracker) == 0
    assert run.step(run.grads())
    assert float(run.scaler.last[3]) == SCALES[mode] / 2


def test_a_skipped_first_step_leaves_no_buffers():
    run = Run("fp16", True, "scale")
    assert not run.step(run.grads(bad=(0, 0, np.nan)))
    assert all("momentum_buffer" not in run.state[p] for p in run.params)
    assert run.step(run.grads())


def test_the_scale_grows_after_growth_interval_taken_steps():
    run = Run("fp32", False, "scale", interval=2)
    for want in (1000.0, 2000.0, 2000.0, 4000.0):
        assert run.step(run.grads())
        assert run.scaler.get_scale() == want
    assert float(run.scaler.last[3]) == 2000.0, "the step ran with the scale before its own update"


@pytest.mark.parametrize("entry", ["loop", "step"])
def test_a_pinned_total_with_loss_scale_raises_and_changes_nothing(entry):
    from chocosgd_amd import utils
    run = Run("bf16", True, "both", entry)
    for p, g in zip(run.params, run.grads()):
        p.grad = torch.from_numpy(g.copy()).to(p.dtype)
    agg = AO.Loopback(3, peers=[[np.zeros(N + 1, np.float32)] * 2])
    before = run.snapshot()
    with pytest.raises(RuntimeError, match="total_norm"):
        run.fn(run.groups, run.names, run.state, agg, master=run.mw, clip_norm=0.4, total_norm=1.0,
               loss_scale=run.scaler)
    with pytest.raises(RuntimeError, match="clip_norm"):  # a pinned total needs a clip
        run.fn(run.groups, run.names, run.state, agg, master=run.mw, total_norm=1.0)
    with pytest.raises(RuntimeError, match="LossScaler"):
        run.fn(run.groups, run.names, run.state, agg, master=run.mw, loss_scale=torch.amp.GradScaler("cpu"))
    assert agg.calls == 0 and run.scaler.last is None
    assert run.scaler.get_scale() == SCALES["bf16"] and int(run.scaler._growth_tracker) == 0
    assert all(same_bits(a, b) for a, b in zip(before, run.snapshot()))
    assert all("momentum_buffer" not in run.state[p] for p in run.params)


def test_not_distributed_keeps_the_local_flag_and_divides_by_one():
    """distributed=False: no collective, divisor 1, flat[n] is the local flag."""
    from chocosgd_amd import utils
    run = Run("fp32", False, "scale")
    for bad, taken in ((None, True), ((8, 5, -np.inf), False)):
        raw = run.grads(bad=bad)
        for p, g in zip(run.params, raw):
            p.grad = torch.from_numpy(g.copy())
        agg = AO.Loopback(5)
        assert utils.allreduce_sgd_step(run.groups, run.names, run.state, agg, distributed=False,
                                        loss_scale=run.scaler) == 32 * (N + 1)
        assert agg.calls == 0
        out = run.mdl.local(raw, None, total=host(run.scaler.last)[0])
        assert run.mdl.apply(run.mdl.flat(raw, out), 1.0) == taken == (not run.scaler.skipped())
        assert same_bits(_cat(run.params), run.mdl.cat("p16"))


# ----------------------------------------------------------------------------- the reference's recorded steps
SETS = ["clip", "nesterov", "damp"]


def fixture_model(inputs, hp, device="cpu"):
    lens = inputs["lens"].tolist()
    params, o = [], 0
    for m in lens:
        params.append(torch.nn.Parameter(torch.from_numpy(inputs["p0"][o:o + m].copy()).to(device)))
        o += m
    groups, names = AO.groups_of(params, tuple(hp))
    return params, groups, names, lens


def replay(fn, device, name, master, how):
    """Rank 0 of the reference's recorded run through `fn`: clip_grad_norm_ then SGD.step, world
    3, the total pinned to what torch returned on that rank."""
    from chocosgd_amd import utils
    inputs, fx = golden("allreduce_clip_inputs"), golden(f"allreduce_clip_{name}")
    hp = fx["hp"].tolist()
    hp[4] = bool(hp[4])
    params, groups, names, lens = fixture_model(inputs, hp, device)
    n = sum(lens)
    if how == "recorded sum":
        agg = AO.Loopback(3, sums=[inputs[f"sum{k}"] for k in range(STEPS)])
    else:
        agg = AO.Loopback(3, peers=[[inputs[f"c1_{k}"], inputs[f"c2_{k}"]] for k in range(STEPS)])
    mw = utils.MasterWeights(groups, names) if master else None
    state = collections.defaultdict(dict)
    for k in range(STEPS):
        o = 0
        for p, m in zip(params, lens):
            p.grad = torch.from_numpy(inputs[f"g{k}"][o:o + m].copy()).to(device)
            o += m
        grads = [p.grad for p in params]
        assert fn(groups, names, state, agg, master=mw, clip_norm=float(inputs["max_norm"]),
                  total_norm=float(inputs[f"total0_{k}"])) == 32 * n
        assert all(p.grad is g for p, g in zip(params, grads)), "p.grad was rebound"
        assert same_bits(_cat(grads), inputs[f"avg{k}"]), f"the averaged gradient after step {k}"
        assert same_bits(_cat(params), fx[f"p{k}"]), f"p after step {k}"
        if master:
            assert same_bits(host(mw.buffer), fx[f"p{k}"]), f"master after step {k}"
        if hp[2] != 0:
            assert same_bits(_cat([state[p]["momentum_buffer"] for p in params]), fx[f"buf{k}"]), f"buf, step {k}"
    assert agg.calls == STEPS
    return agg


def test_the_fixtures_hold_what_the_issue_asks_for():
    """World 3; every rank's step 0 is clipped and step 2 is not; the recorded sum is rank 0's
    clipped gradient plus the peers' in the generator's order; the model's clip of rank 0's raw
    gradient at torch's total is what went into it."""
    inputs = golden("allreduce_clip_inputs")
    assert float(inputs["world"]) == 3.0
    mx = float(inputs["max_norm"])
    for k in range(STEPS):
        for r in range(3):
            t = float(inputs[f"total{r}_{k}"])
            assert (t > 10 * mx) if k == 0 else (t < 0.1 * mx) if k == 2 else True
        c = GO.coef(inputs[f"total0_{k}"], mx)
        assert (c < 1) == (k < 2)
        own = GO.clip(inputs[f"g{k}"], c)
        assert same_bits(ASO.add([own, inputs[f"c1_{k}"], inputs[f"c2_{k}"]]), inputs[f"sum{k}"])
        assert same_bits(AO.fdiv(inputs[f"sum{k}"], 3.0), inputs[f"avg{k}"])


@pytest.mark.parametrize("how", ["recorded sum", "peers added"])
@pytest.mark.parametrize("master", [False, True], ids=["plain", "master"])
@pytest.mark.parametrize("name", SETS)
def test_fixture_replay_on_cpu_tensors(name, master, how):
    from chocosgd_amd import utils
    agg = replay(utils.allreduce_sgd_step, "cpu", name, master, how)
    inputs = golden("allreduce_clip_inputs")
    for k in range(STEPS):
        c = GO.coef(inputs[f"total0_{k}"], float(inputs["max_norm"]))
        assert same_bits(agg.seen[k], GO.clip(inputs[f"g{k}"], c)), "the packed, clipped gradients"


# ----------------------------------------------------------------------------- argument checks
ERR_INVALID = -1  # CHOCO_ERR_INVALID


@pytest.fixture(scope="module")
def lib():
    from chocosgd_amd import _lib
    return _lib.load()


def _tables(k=1, m=4):
    arr = lambda ct, vals: (ct * k)(*vals)  # noqa: E731
    return (arr(ctypes.c_void_p, [0x1000 + 0x100 * i for i in range(k)]), arr(ctypes.c_int64, [m] * k),
            arr(ctypes.c_int32, [0] * k))


PACK_BAD = {
    "null coef": (dict(coef=0), "coef"),
    "coef at 2 mod 4": (dict(coef=0x5002), "coef"),
    "found at 2 mod 4": (dict(found=0x6002), "found"),
    "round 2": (dict(round=2), "round"),
    "round -1": (dict(round=-1), "round"),
    "null flat": (dict(flat=0), "flat"),
    "flat at 2 mod 4": (dict(flat=0x4002), "flat"),
    "lengths": (dict(n=5), "add up"),
    "nseg zero": (dict(nseg=0), "nseg"),
}


@pytest.mark.parametrize("case", sorted(PACK_BAD))
def test_pack_scaled_rejects(lib, case):
    from chocosgd_amd import _lib
    kw, msg = PACK_BAD[case]
    a = dict(flat=0x4000, n=4, coef=0x5000, found=0x6000, round=1, nseg=1)
    a.update(kw)
    ptrs, lens, dts = _tables()
    rc = lib.choco_params_pack_scaled(ptrs, lens, dts, a["nseg"], ctypes.c_void_p(a["flat"]), a["n"],
                                      ctypes.c_void_p(a["coef"]), ctypes.c_void_p(a["found"]), a["round"], None)
    assert rc == ERR_INVALID and msg in _lib.last_error(), (case, _lib.last_error())


STATE_BAD = {
    "null scale": (dict(scale=0), "scale_state"),
    "scale at 2 mod 4": (dict(scale=0x7002), "scale_state"),
    "null tracker": (dict(tracker=0), "growth_tracker"),
    "tracker at 2 mod 4": (dict(tracker=0x8002), "growth_tracker"),
    "growth 1": (dict(growth=1.0), "growth"),
    "growth inf": (dict(growth=float("inf")), "growth"),
    "growth nan": (dict(growth=float("nan")), "growth"),
    "backoff 0": (dict(backoff=0.0), "backoff"),
    "backoff 1": (dict(backoff=1.0), "backoff"),
    "interval 0": (dict(interval=0), "interval"),
    "null out": (dict(out=0), "out"),
    "out at 2 mod 4": (dict(out=0x9002), "out"),
}


@pytest.mark.parametrize("case", sorted(STATE_BAD) + ["null found_sum", "found_sum at 2 mod 4"])
def test_loss_scale_update_rejects(lib, case):
    from chocosgd_amd import _lib
    a = dict(found=0xa000, scale=0x7000, tracker=0x8000, growth=2.0, backoff=0.5, interval=2000, out=0x9000)
    if case in STATE_BAD:
        kw, msg = STATE_BAD[case]
    else:
        kw, msg = dict(found=0 if case.startswith("null") else 0xa002), "found_sum"
    a.update(kw)
    rc = lib.choco_loss_scale_update(ctypes.c_void_p(a["found"]), ctypes.c_void_p(a["scale"]),
                                     ctypes.c_void_p(a["tracker"]), a["growth"], a["backoff"], a["interval"],
                                     ctypes.c_void_p(a["out"]), None)
    assert rc == ERR_INVALID and msg in _lib.last_error(), (case, _lib.last_error())


@pytest.mark.parametrize("case", sorted(STATE_BAD) + ["has_clip 2", "max_norm nan"])
def test_gradnorm_scaled_local_rejects_what_gradnorm_scaled_rejects(lib, case):
    from chocosgd_amd import _lib
    a = dict(scale=0x7000, tracker=0x8000, growth=2.0, backoff=0.5, interval=2000, out=0x9000, has_clip=1,
             max_norm=0.4)
    kw, msg = STATE_BAD[case] if case in STATE_BAD else \
        (dict(has_clip=2), "has_clip") if case == "has_clip 2" else (dict(max_norm=float("nan")), "max_norm")
    a.update(kw)
    ptrs, lens, dts = _tables()
    flags = (ctypes.c_int32 * 1)(0)
    for fn in (lib.choco_params_gradnorm_scaled_local, lib.choco_params_gradnorm_scaled):
        rc = fn(ptrs, lens, dts, flags, 1, 4, a["max_norm"], 0, ctypes.c_void_p(a["scale"]),
                ctypes.c_void_p(a["tracker"]), a["growth"], a["backoff"], a["interval"], a["has_clip"],
                ctypes.c_void_p(a["out"]), None, ctypes.c_void_p(0xb000), 1 << 20, None)
        assert rc == ERR_INVALID and msg in _lib.last_error(), (case, _lib.last_error())


def test_flatgrad_scaled_rejects_what_flatgrad_rejects(lib):
    """The unscaled entry points' checks apply; gsum may not be null even at n == 0."""
    from chocosgd_amd import _lib
    k = 1
    arr = lambda ct, vals: (ct * k)(*vals)  # noqa: E731
    tabs = [arr(ctypes.c_void_p, [0x1000]), arr(ctypes.c_void_p, [0x2000]), arr(ctypes.c_void_p, [0x3000]),
            arr(ctypes.c_int64, [4]), arr(ctypes.c_int32, [0]), arr(ctypes.c_double, [0.1]),
            arr(ctypes.c_double, [0.0]), arr(ctypes.c_double, [0.0]), arr(ctypes.c_double, [0.0]),
            arr(ctypes.c_int32, [0])]
    for gsum, n, divisor, mode, msg in [(0, 4, 3.0, 6, "gsum"), (0x20002, 4, 3.0, 6, "gsum"),
                                        (0x20000, 4, 0.0, 6, "divisor"), (0x20000, 4, 3.0, 1, "apply mode"),
                                        (0x20000, 5, 3.0, 6, "add up")]:
        rc = lib.choco_params_sgd_flatgrad_scaled(*tabs, k, ctypes.c_void_p(gsum), n, divisor, mode, None)
        assert rc == ERR_INVALID and msg in _lib.last_error(), (msg, _lib.last_error())
        rc = lib.choco_params_sgd_master_flatgrad_scaled(*tabs, k, ctypes.c_void_p(gsum), ctypes.c_void_p(0x10000), n,
                                                         divisor, mode, None)
        assert rc == ERR_INVALID and msg in _lib.last_error(), (msg, _lib.last_error())
    rc = lib.choco_params_sgd_master_flatgrad_scaled(*tabs, k, ctypes.c_void_p(0x20000), None, 4, 3.0, 6, None)
    assert rc == ERR_INVALID and "master" in _lib.last_error()
    tabs[3] = arr(ctypes.c_int64, [0])
    rc = lib.choco_params_sgd_flatgrad_scaled(*tabs, k, None, 0, 3.0, 6, None)
    assert rc == ERR_INVALID and "gsum" in _lib.last_error(), "the flag slot has to exist"
