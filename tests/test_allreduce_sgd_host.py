"""The all-reduce SGD step, host side (no GPU): the argument checks of
choco_params_sgd_flatgrad / choco_params_sgd_master_flatgrad, made before any HIP call; the
launch count rule; utils.allreduce_sgd_step on CPU tensors (the loop path) and the numpy model
(tests/_allreduce_oracle.py) against the reference's own recorded steps
(tests/golden/allreduce_sgd_*.npz, world 3), bit for bit; the 16-bit steps against the model;
the bf16 tie the master step keeps; the lost-update case; the Python refusals."""
import collections
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden, same_bits
import _allreduce_oracle as AO
import _master_oracle as MA
import _sgd_oracle as SO

ERR_INVALID = -1  # CHOCO_ERR_INVALID
F32, BF16, F16 = 0, 1, 2
NESTEROV, FIRST, NOGRAD = 1, 2, 4
APPLY, GRAD, WRITE_PARAMS, WRITE_GRADS, ADD_FLAT = 0, 1, 2, 4, 8
STEPS = 3
SETS = ["plain", "wd", "mom", "nesterov", "damp"]
HPS = {"plain": (0.1, 0.0, 0.0, 0.0, False), "wd": (0.05, 1e-4, 0.0, 0.0, False), "mom": (0.1, 0.0, 0.9, 0.0, False),
       "damp": (0.01, 1e-4, 0.9, 0.1, False), "nesterov": (0.1, 5e-4, 0.9, 0.0, True)}


@pytest.fixture(scope="module")
def lib():
    from chocosgd_amd import _lib
    return _lib.load()


# ----------------------------------------------------------------------------- argument checks
def _call(lib, p, g, b, lens, dts, n, lr=None, wd=None, mom=None, damp=None, flags=None, gsum=0x20000, master=None,
          divisor=3.0, mode=WRITE_PARAMS | WRITE_GRADS, nseg=None, null=(), msg=None):
    """One call with host tables built from the lists; the made-up device pointers are never
    dereferenced (every case here is rejected before the first launch).  master: None takes
    choco_params_sgd_flatgrad, an address choco_params_sgd_master_flatgrad."""
    k = len(p)
    arr = lambda ct, vals: (ct * max(k, 1))(*vals)  # noqa: E731
    tabs = {"params": arr(ctypes.c_void_p, p), "grads": arr(ctypes.c_void_p, g), "bufs": arr(ctypes.c_void_p, b),
            "lens": arr(ctypes.c_int64, lens), "dtypes": arr(ctypes.c_int32, dts),
            "lr": arr(ctypes.c_double, lr or [0.1] * k), "wd": arr(ctypes.c_double, wd or [0.0] * k),
            "mom": arr(ctypes.c_double, mom or [0.0] * k), "damp": arr(ctypes.c_double, damp or [0.0] * k),
            "flags": arr(ctypes.c_int32, flags or [0] * k)}
    a = [None if nm in null else t for nm, t in tabs.items()]
    a += [k if nseg is None else nseg, ctypes.c_void_p(gsum)]
    if master is None:
        return lib.choco_params_sgd_flatgrad(*a, n, divisor, mode, None)
    return lib.choco_params_sgd_master_flatgrad(*a, ctypes.c_void_p(master), n, divisor, mode, None)


ONE = dict(p=[0x1000], g=[0x2000], b=[0x3000], lens=[4], dts=[F32], n=4)
TWO = dict(p=[0x1000, 0x1100], g=[0x2000, 0x2100], b=[0x3000, 0x3100], lens=[4, 4], dts=[F32, BF16], n=8)
BOTH = {  # refused by both entry points
    **{f"null {t}": dict(ONE, null=(t,), msg="null table")
       for t in ["params", "bufs", "lens", "dtypes", "lr", "wd", "mom", "damp", "flags"]},
    "grad mode": dict(ONE, mode=GRAD, msg="apply mode"),
    "grad mode writing grads": dict(ONE, mode=GRAD | WRITE_GRADS, msg="apply mode"),
    "add flat": dict(ONE, mode=ADD_FLAT | WRITE_PARAMS, msg="unknown mode"),
    "unknown mode bit": dict(ONE, mode=16 | WRITE_PARAMS, msg="unknown mode"),
    "no-grad tensor": dict(TWO, flags=[0, NOGRAD], msg="no-grad"),
    "no-grad tensor without the grad write": dict(TWO, flags=[NOGRAD, 0], mode=WRITE_PARAMS, msg="no-grad"),
    "write grads, null grads table": dict(ONE, null=("grads",), msg="WRITE_GRADS"),
    "write grads, null grad pointer": dict(TWO, g=[0x2000, 0], msg="null grad pointer"),
    "divisor zero": dict(ONE, divisor=0.0, msg="divisor"),
    "divisor zero as fp32": dict(ONE, divisor=1e-60, msg="divisor"),
    "divisor infinite": dict(ONE, divisor=float("inf"), msg="divisor"),
    "divisor infinite as fp32": dict(ONE, divisor=1e39, msg="divisor"),
    "divisor nan": dict(ONE, divisor=float("nan"), msg="divisor"),
    "null gsum": dict(ONE, gsum=0, msg="gsum"),
    "gsum at 2 mod 4": dict(ONE, gsum=0x20002, msg="gsum"),
    "nseg zero": dict(ONE, nseg=0, msg="nseg"),
    "dtype 3": dict(ONE, dts=[3], msg="dtype"),
    "sum below n": dict(TWO, n=9, msg="add up"),
    "sum above n": dict(TWO, n=7, msg="add up"),
    "negative length": dict(TWO, lens=[-4, 8], n=4, msg="negative length"),
    "nesterov without momentum": dict(ONE, flags=[NESTEROV], mom=[0.0], msg="nesterov"),
    "nesterov with dampening": dict(ONE, flags=[NESTEROV], mom=[0.9], damp=[0.1], msg="nesterov"),
    "null buf with momentum": dict(TWO, b=[0x3000, 0], mom=[0.9, 0.9], msg="null momentum buffer"),
    "fp32 param at 2 mod 4": dict(TWO, p=[0x1002, 0x1100], msg="aligned"),
    "bf16 grad at odd byte": dict(TWO, g=[0x2000, 0x2101], msg="aligned"),
    "fp32 buf at 2 mod 4": dict(TWO, b=[0x3002, 0x3100], msg="aligned"),
    "null param": dict(TWO, p=[0x1000, 0], msg="null param"),
    "unknown flag bit": dict(ONE, flags=[8], msg="flag"),
}
MASTER_ONLY = {
    "null master": dict(ONE, master=0, msg="master"),
    "master at 2 mod 4": dict(ONE, master=0x10002, msg="master"),
    "bf16 tensor, 16-bit buf at 2 mod 4": dict(TWO, master=0x10000, b=[0x3000, 0x3102], mom=[0.9, 0.9], msg="aligned"),
    "fp16 tensor, 16-bit buf at 2 mod 4": dict(TWO, master=0x10000, dts=[F32, F16], b=[0x3000, 0x3102], msg="aligned"),
}
BAD = {**{f"plain: {k}": v for k, v in BOTH.items()},
       **{f"master: {k}": dict(v, master=0x10000) for k, v in BOTH.items()},
       **{f"master: {k}": v for k, v in MASTER_ONLY.items()}}


@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_arguments_are_rejected(lib, case):
    from chocosgd_amd import _lib
    assert _call(lib, **BAD[case]) == ERR_INVALID, case
    err = _lib.last_error()
    assert err != "" and BAD[case]["msg"] in err, (case, err)


def test_what_the_checks_let_through(lib):
    """A 16-bit buffer at 2 mod 4 is fine in the plain call; a null grads table, or a null grad
    pointer, is fine without WRITE_GRADS.  (Each call is still rejected, later, for its
    lengths: nothing is launched.)"""
    from chocosgd_amd import _lib
    for kw in (dict(TWO, b=[0x3000, 0x3102], mom=[0.9, 0.9]), dict(TWO, null=("grads",), mode=WRITE_PARAMS),
               dict(TWO, g=[0, 0], mode=WRITE_PARAMS), dict(TWO, g=[0, 0], mode=APPLY, master=0x10000),
               dict(TWO, divisor=1.0), dict(TWO, divisor=-2.0)):
        assert _call(lib, **dict(kw, n=9)) == ERR_INVALID
        assert "add up" in _lib.last_error(), kw


def test_launches_rule(lib):
    from chocosgd_amd import codec
    cap = max(k for k in range(1, 1024) if lib.choco_params_sgd_flatgrad_launches(k) == 1)
    assert cap == 72  # the table of choco_params_sgd
    for nseg in [1, cap - 1, cap, cap + 1, 2 * cap + 3, 3000]:
        assert lib.choco_params_sgd_flatgrad_launches(nseg) == -(-nseg // cap), nseg
        assert codec.params_sgd_flatgrad_launches(nseg) == -(-nseg // cap)
    assert lib.choco_params_sgd_flatgrad_launches(161) == 3
    assert lib.choco_params_sgd_flatgrad_launches(0) == 0 and lib.choco_params_sgd_flatgrad_launches(-4) == 0


# ----------------------------------------------------------------------------- the reference's recorded steps
def _fixture_model(inputs, hp, dtype=torch.float32):
    lens = inputs["lens"].tolist()
    params, o = [], 0
    for m in lens:
        params.append(torch.nn.Parameter(torch.from_numpy(inputs["p0"][o:o + m].copy()).to(dtype)))
        o += m
    groups, names = AO.groups_of(params, tuple(hp))
    return params, groups, names, lens


def _set_grads(params, lens, flat):
    o = 0
    for p, m in zip(params, lens):
        p.grad = torch.from_numpy(flat[o:o + m].copy()).to(p.dtype)
        o += m


def _cat(tensors):
    return np.concatenate([MA.host(t).reshape(-1) for t in tensors])


def test_the_fixtures_hold_what_the_issue_asks_for():
    """World 3; sums with NaN from inf + -inf, subnormal sums, and a third of the finite
    averages differing from a reciprocal multiply."""
    sums = golden("allreduce_sgd_sums")
    assert float(sums["world"]) == 3.0
    for k in range(STEPS):
        s, a = sums[f"sum{k}"], sums[f"avg{k}"]
        with np.errstate(all="ignore"):
            recip = (s * np.float32(1.0 / 3.0)).astype(np.float32)
            sub = np.isfinite(s) & (s != 0) & (np.abs(s) < np.float32(2.0 ** -126))
        assert np.isnan(s).sum() >= 2 and sub.sum() >= 2
        differ = np.isfinite(a) & (recip.view(np.uint32) != a.view(np.uint32))
        assert differ.sum() > s.size // 4


@pytest.mark.parametrize("how", ["recorded sum", "peers added"])
@pytest.mark.parametrize("master", [False, True])
@pytest.mark.parametrize("name", SETS)
def test_fixture_replay_on_cpu_tensors(name, master, how):
    """allreduce_sgd_step on CPU tensors (the loop) as rank 0 of the reference's recorded run:
    the loopback aggregator returns the recorded sum, or adds the two peers' recorded gradients
    as the generator's all_reduce did.  With fp32 tensors the master step is the plain one."""
    from chocosgd_amd import utils
    inputs, peers, sums, fx = (golden(nm) for nm in ("sgd_inputs", "allreduce_sgd_peers", "allreduce_sgd_sums",
                                                     f"allreduce_sgd_{name}"))
    hp = fx["hp"].tolist()
    params, groups, names, lens = _fixture_model(inputs, hp)
    n = sum(lens)
    if how == "recorded sum":
        agg = AO.Loopback(3, sums=[sums[f"sum{k}"] for k in range(STEPS)])
    else:
        agg = AO.Loopback(3, peers=[[peers[f"q1_{k}"], peers[f"q2_{k}"]] for k in range(STEPS)])
    mw = utils.MasterWeights(groups, names) if master else None
    state = collections.defaultdict(dict)
    for k in range(STEPS):
        _set_grads(params, lens, inputs[f"g{k}"])
        grads = [p.grad for p in params]
        assert utils.allreduce_sgd_step(groups, names, state, agg, master=mw) == 32 * n
        assert same_bits(agg.seen[k], inputs[f"g{k}"]), "the packed gradients"
        assert all(p.grad is g for p, g in zip(params, grads)), "p.grad was rebound"
        assert same_bits(_cat(grads), sums[f"avg{k}"]), f"the averaged gradient after step {k}"
        assert same_bits(_cat(params), fx[f"p{k}"]), f"p after step {k}"
        if master:
            assert same_bits(MA.host(mw.buffer), fx[f"p{k}"]), f"master after step {k}"
        if hp[2] != 0:
            assert same_bits(_cat([state[p]["momentum_buffer"] for p in params]), fx[f"buf{k}"]), f"buf, step {k}"
    assert agg.calls == STEPS


@pytest.mark.parametrize("name", SETS)
def test_the_model_against_the_fixtures(name):
    """to_grid(fdiv(sum, w)) then _sgd_oracle.sgd_step, and the master model, against the
    reference's recorded sums, averages, parameters and buffers."""
    inputs, peers, sums, fx = (golden(nm) for nm in ("sgd_inputs", "allreduce_sgd_peers", "allreduce_sgd_sums",
                                                     f"allreduce_sgd_{name}"))
    lr, wd, mom, damp, nest = fx["hp"].tolist()
    w = float(sums["world"])
    p = m = inputs["p0"]
    buf = mbuf = None
    for k in range(STEPS):
        with np.errstate(all="ignore"):
            s = ((inputs[f"g{k}"] + peers[f"q1_{k}"]).astype(np.float32) + peers[f"q2_{k}"]).astype(np.float32)
        assert same_bits(s, sums[f"sum{k}"]), "the fixed order of the generator's all_reduce"
        assert same_bits(AO.fdiv(s, w), sums[f"avg{k}"])
        p, buf, g = AO.step(p, s, buf, w, lr, wd, mom, damp, bool(nest), first=k == 0)
        m, mbuf, p16, g16 = AO.master_step(m, s, mbuf, w, lr, wd, mom, damp, bool(nest), first=k == 0)
        assert same_bits(g, sums[f"avg{k}"]) and same_bits(g16, sums[f"avg{k}"])
        assert same_bits(p, fx[f"p{k}"]) and same_bits(m, fx[f"p{k}"]) and same_bits(p16, fx[f"p{k}"])
        if mom != 0:
            assert same_bits(buf, fx[f"buf{k}"]) and same_bits(mbuf, fx[f"buf{k}"])


# ----------------------------------------------------------------------------- the loop in 16 bits
LENS = [1, 2, 3, 7, 8, 9, 31, 33, 300]


def _dtypes(mode, k):
    return [MA.DTYPES[mode] if mode != "mixed" else list(MA.DTYPES.values())[i % 3] for i in range(k)]


def _model(mode, hp, seed=0):
    rng = np.random.RandomState(seed)
    dts = _dtypes(mode, len(LENS))
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(m).astype(np.float32)).to(dt))
              for m, dt in zip(LENS, dts)]
    groups, names = AO.groups_of(params, hp)
    return params, groups, names, dts, rng


@pytest.mark.parametrize("entry", ["loop", "step"])
@pytest.mark.parametrize("write_grads", [True, False])
@pytest.mark.parametrize("master", [False, True])
@pytest.mark.parametrize("name", sorted(HPS))
@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32", "mixed"])
def test_cpu_loop_matches_the_model(mode, name, master, write_grads, entry):
    """Three steps of world 3: parameters, buffers, grads and (master) the master copy after
    every step.  CPU tensors take the loop through utils.allreduce_sgd_step as well."""
    from chocosgd_amd import utils
    hp = HPS[name]
    params, groups, names, dts, rng = _model(mode, hp)
    n = sum(LENS)
    mw = utils.MasterWeights(groups, names) if master else None
    state = collections.defaultdict(dict)
    cur = [MA.host(p) for p in params]  # the master copy, or the parameters
    bufs = [None] * len(params)
    fn = utils.allreduce_sgd_step_loop if entry == "loop" else utils.allreduce_sgd_step
    for k in range(STEPS):
        own = [SO.to_grid((0.1 * rng.standard_normal(m)).astype(np.float32), MA.NAMES[dt]) for m, dt in zip(LENS, dts)]
        peers = [(0.1 * rng.standard_normal(n)).astype(np.float32) for _ in range(2)]
        for p, g in zip(params, own):
            p.grad = torch.from_numpy(g.copy()).to(p.dtype)
        with np.errstate(all="ignore"):
            s = ((np.concatenate(own) + peers[0]).astype(np.float32) + peers[1]).astype(np.float32)
        agg = AO.Loopback(3, peers=[peers])
        assert fn(groups, names, state, agg, write_grads=write_grads, master=mw) == 32 * n
        assert agg.calls == 1 and same_bits(agg.seen[0], np.concatenate(own)), "the widened gradients"
        o = 0
        for i, (p, dt) in enumerate(zip(params, dts)):
            si = s[o:o + LENS[i]]
            o += LENS[i]
            if master:
                cur[i], bufs[i], want_p, want_g = AO.master_step(cur[i], si, bufs[i], 3.0, *hp, first=k == 0,
                                                                 dtype=MA.NAMES[dt])
            else:
                cur[i], bufs[i], want_g = AO.step(cur[i], si, bufs[i], 3.0, *hp, first=k == 0, dtype=MA.NAMES[dt])
                want_p = cur[i]
            assert same_bits(MA.host(p), want_p), f"param {i} after step {k}"
            assert same_bits(MA.host(p.grad), want_g if write_grads else own[i]), f"grad {i} after step {k}"
            if hp[2] != 0:
                buf = state[p]["momentum_buffer"]
                assert buf.dtype == (torch.float32 if master else dt) and same_bits(MA.host(buf), bufs[i]), (i, k)
            else:
                assert "momentum_buffer" not in state[p]
        if master:
            assert same_bits(MA.host(mw.buffer), np.concatenate(cur)), f"master after step {k}"


def test_not_distributed_divides_by_one():
    """distributed=False: _agg hands the buffer back (communication.py:169-170) and the divisor
    is 1.0 whatever the world size says: the plain apply_gradient on the local gradients."""
    from chocosgd_amd import utils
    hp = HPS["damp"]
    params, groups, names, dts, rng = _model("fp32", hp)
    twin = [torch.nn.Parameter(p.detach().clone()) for p in params]
    tgroups, _ = AO.groups_of(twin, hp)
    for p, q in zip(params, twin):
        p.grad = torch.from_numpy((0.1 * rng.standard_normal(p.numel())).astype(np.float32)).to(p.dtype)
        q.grad = p.grad.clone()
    agg = AO.Loopback(5)
    state, tstate = collections.defaultdict(dict), collections.defaultdict(dict)
    utils.allreduce_sgd_step(groups, names, state, agg, distributed=False)
    utils.apply_gradient_loop(tgroups, tstate, True)
    assert agg.calls == 0
    for p, q in zip(params, twin):
        assert same_bits(MA.host(p), MA.host(q)) and same_bits(MA.host(p.grad), MA.host(q.grad))
        assert same_bits(MA.host(state[p]["momentum_buffer"]), MA.host(tstate[q]["momentum_buffer"]))


# ----------------------------------------------------------------------------- what the master keeps
def test_bf16_average_on_a_tie():
    """World 2, the two ranks' gradients 1.0 and 1 + 2^-7 (both bf16 values): the sum 2 + 2^-7
    and the average 1 + 2^-8 are exact in fp32; the average is the tie between the bf16
    neighbours 1.0 (even) and 1 + 2^-7.  The 16-bit step's g is 1.0; the master step keeps
    1 + 2^-8.  lr = 0.5 on p = 2: 1.5 against 1.5 - 2^-9 in the master."""
    from chocosgd_amd import utils
    m = 37
    tie = 1.0 + 2.0 ** -8
    assert float(np.float32(tie)) == tie and SO.to_grid(np.float32([tie]), "bf16")[0] == 1.0
    for use_master in (False, True):
        p = torch.nn.Parameter(torch.full((m,), 2.0, dtype=torch.bfloat16))
        p.grad = torch.ones(m, dtype=torch.bfloat16)
        groups, names = AO.groups_of([p], (0.5, 0.0, 0.0, 0.0, False))
        mw = utils.MasterWeights(groups, names) if use_master else None
        agg = AO.Loopback(2, peers=[[np.full(m, 1.0 + 2.0 ** -7, dtype=np.float32)]])
        utils.allreduce_sgd_step(groups, names, collections.defaultdict(dict), agg, master=mw)
        assert same_bits(MA.host(p.grad), np.full(m, 1.0, dtype=np.float32)), "the bf16 gradient: the tie goes to even"
        if use_master:
            want = np.full(m, 1.5 - 2.0 ** -9, dtype=np.float32)
            assert same_bits(MA.host(mw.buffer), want), "the master step used 1 + 2^-8"
            assert same_bits(AO.master_step(np.full(m, 2.0, np.float32), np.full(m, 2.0 + 2.0 ** -7, np.float32), None,
                                            2.0, 0.5, dtype="bf16")[0], want)
            assert same_bits(MA.host(p), SO.to_grid(want, "bf16"))
        else:
            assert same_bits(MA.host(p), np.full(m, 1.5, dtype=np.float32)), "the 16-bit step used 1.0"


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_cpu_lost_updates(name):
    AO.check_lost_updates(name, "cpu", same_bits)


# ----------------------------------------------------------------------------- refusals
def test_cpu_refusals_change_nothing():
    from chocosgd_amd import utils
    params, groups, names, _, rng = _model("bf16", HPS["mom"])
    for p in params:
        p.grad = torch.ones_like(p)
    mw = utils.MasterWeights(groups, names)
    state = collections.defaultdict(dict)
    agg = AO.Loopback(3, peers=[[np.zeros(sum(LENS), np.float32)] * 2] * 8)

    def snapshot():
        return [mw.buffer.clone()] + [p.detach().clone() for p in params] + [p.grad.clone() for p in params]

    snap = snapshot()
    state[params[3]]["momentum_buffer"] = torch.zeros_like(params[3])  # a bf16 buffer of the 16-bit step
    for fn in (utils.allreduce_sgd_step, utils.allreduce_sgd_step_loop):
        with pytest.raises(RuntimeError, match="float32 momentum buffers"):
            fn(groups, names, state, agg, master=mw)
    del state[params[3]]["momentum_buffer"]
    other = utils.MasterWeights(groups[:-1], names[:-1])  # built for another (smaller) model
    foreign = utils.MasterWeights(groups, names[::-1])    # built for other param_names
    for fn in (utils.allreduce_sgd_step, utils.allreduce_sgd_step_loop):
        with pytest.raises(RuntimeError):
            fn(groups, names, state, agg, master=other)
        with pytest.raises(RuntimeError, match="param_names"):
            fn(groups, names, state, agg, master=foreign)
        with pytest.raises(RuntimeError):  # a group named twice
            fn(groups, names[:-1] + names[:1], state, agg)
    kept, params[2].grad = params[2].grad, None
    for fn in (utils.allreduce_sgd_step, utils.allreduce_sgd_step_loop):
        for m in (None, mw):
            with pytest.raises(RuntimeError, match="no gradient"):  # the flat gradient has no slot to skip
                fn(groups, names, state, agg, master=m)
    params[2].grad = kept
    assert agg.calls == 0, "a refused step reached the all-reduce"
    assert all(torch.equal(a, b) for a, b in zip(snap, snapshot()))
    assert all("momentum_buffer" not in state[p] for p in params)
