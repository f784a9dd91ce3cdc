"""The SGD update on fp32 master weights, host side (no GPU): the argument checks of
choco_params_sgd_master, made before any HIP call; the launch count rule;
utils.apply_gradient_master_loop on CPU tensors against the numpy model (tests/_master_oracle.py)
and the reference's fp32 fixtures, bit for bit; the lost-update case."""
import collections
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden, same_bits
import _master_oracle as MA
import _sgd_oracle as SO

ERR_INVALID = -1  # CHOCO_ERR_INVALID
F32, BF16, F16 = 0, 1, 2
NESTEROV, FIRST, NOGRAD = 1, 2, 4
APPLY, GRAD, WRITE_PARAMS, WRITE_GRADS, ADD_FLAT = 0, 1, 2, 4, 8
STEPS = 3
HPS = {"plain": (0.1, 0.0, 0.0, 0.0, False), "wd": (0.05, 1e-4, 0.0, 0.0, False), "mom": (0.1, 0.0, 0.9, 0.0, False),
       "damp": (0.01, 1e-4, 0.9, 0.1, False), "nesterov": (0.1, 5e-4, 0.9, 0.0, True)}


@pytest.fixture(scope="module")
def lib():
    from chocosgd_amd import _lib
    return _lib.load()


# ----------------------------------------------------------------------------- argument checks
def _call(lib, p, g, b, lens, dts, n, lr=None, wd=None, mom=None, damp=None, flags=None, master=0x10000,
          mode=WRITE_PARAMS, nseg=None, null=(), msg=None):
    """One call with host tables built from the lists; the made-up device pointers are never
    dereferenced (every case here is rejected before the first launch)."""
    k = len(p)
    arr = lambda ct, vals: (ct * max(k, 1))(*vals)  # noqa: E731
    tabs = {"params": arr(ctypes.c_void_p, p), "grads": arr(ctypes.c_void_p, g), "bufs": arr(ctypes.c_void_p, b),
            "lens": arr(ctypes.c_int64, lens), "dtypes": arr(ctypes.c_int32, dts),
            "lr": arr(ctypes.c_double, lr or [0.1] * k), "wd": arr(ctypes.c_double, wd or [0.0] * k),
            "mom": arr(ctypes.c_double, mom or [0.0] * k), "damp": arr(ctypes.c_double, damp or [0.0] * k),
            "flags": arr(ctypes.c_int32, flags or [0] * k)}
    a = [None if nm in null else t for nm, t in tabs.items()]
    return lib.choco_params_sgd_master(*a, k if nseg is None else nseg, ctypes.c_void_p(master), n, mode, None)


ONE = dict(p=[0x1000], g=[0x2000], b=[0x3000], lens=[4], dts=[F32], n=4)
TWO = dict(p=[0x1000, 0x1100], g=[0x2000, 0x2100], b=[0x3000, 0x3100], lens=[4, 4], dts=[F32, BF16], n=8)
BAD = {
    **{f"null {t}": dict(ONE, null=(t,), msg="null table")
       for t in ["params", "grads", "bufs", "lens", "dtypes", "lr", "wd", "mom", "damp", "flags"]},
    "null master": dict(ONE, master=0, msg="master"),
    "null master, nothing written": dict(ONE, master=0, mode=APPLY, msg="master"),
    "master at 2 mod 4": dict(ONE, master=0x10002, msg="4-byte"),
    "grad mode": dict(ONE, mode=GRAD, msg="mode"),
    "grad mode writing grads": dict(ONE, mode=GRAD | WRITE_GRADS, msg="mode"),
    "write grads": dict(ONE, mode=WRITE_GRADS, msg="mode"),
    "add flat": dict(ONE, mode=ADD_FLAT | WRITE_PARAMS, msg="mode"),
    "unknown mode bit": dict(ONE, mode=16, msg="mode"),
    "nseg zero": dict(ONE, nseg=0, msg="nseg"),
    "dtype 3": dict(ONE, dts=[3], msg="dtype"),
    "dtype -1": dict(TWO, dts=[F32, -1], msg="dtype"),
    "sum below n": dict(TWO, n=9, msg="add up"),
    "sum above n": dict(TWO, n=7, msg="add up"),
    "negative length": dict(TWO, lens=[-4, 8], n=4, msg="negative length"),
    "nesterov without momentum": dict(ONE, flags=[NESTEROV], mom=[0.0], msg="nesterov"),
    "nesterov with dampening": dict(ONE, flags=[NESTEROV], mom=[0.9], damp=[0.1], msg="nesterov"),
    "null buf with momentum": dict(TWO, b=[0x3000, 0], mom=[0.9, 0.9], msg="null momentum buffer"),
    "bf16 tensor, buf at 2 mod 4": dict(TWO, b=[0x3000, 0x3102], mom=[0.9, 0.9], msg="aligned"),
    "fp16 tensor, buf at 2 mod 4": dict(TWO, dts=[F32, F16], b=[0x3000, 0x3102], msg="aligned"),
    "bf16 grad at odd byte": dict(TWO, g=[0x2000, 0x2101], msg="aligned"),
    "null param": dict(TWO, p=[0x1000, 0], msg="null param"),
    "null grad": dict(TWO, g=[0, 0x2100], msg="null grad"),
    "unknown flag bit": dict(ONE, flags=[8], msg="flag"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_arguments_are_rejected(lib, case):
    from chocosgd_amd import _lib
    assert _call(lib, **BAD[case]) == ERR_INVALID, case
    err = _lib.last_error()
    assert err != "" and BAD[case]["msg"] in err, (case, err)


def test_a_16bit_param_and_grad_at_2_mod_4_pass_the_alignment_check(lib):
    """Only the buffer is fp32: the tensor's own sides keep their element's alignment.  (The
    call is still rejected, later, for its lengths: nothing is launched.)"""
    from chocosgd_amd import _lib
    assert _call(lib, **dict(TWO, p=[0x1000, 0x1102], g=[0x2000, 0x2102], n=9)) == ERR_INVALID
    assert "add up" in _lib.last_error()


def test_launches_rule(lib):
    from chocosgd_amd import codec
    cap = max(k for k in range(1, 1024) if lib.choco_params_sgd_master_launches(k) == 1)
    assert cap == 72  # the table of choco_params_sgd
    for nseg in [1, cap - 1, cap, cap + 1, 2 * cap + 3, 3000]:
        assert lib.choco_params_sgd_master_launches(nseg) == -(-nseg // cap), nseg
        assert codec.params_sgd_master_launches(nseg) == -(-nseg // cap)
    assert lib.choco_params_sgd_master_launches(161) == 3
    assert lib.choco_params_sgd_master_launches(0) == 0 and lib.choco_params_sgd_master_launches(-4) == 0


# ----------------------------------------------------------------------------- the loop on CPU tensors
LENS = [1, 2, 3, 7, 8, 9, 31, 33, 300]


def _dtypes(mode, k):
    return [MA.DTYPES[mode] if mode != "mixed" else list(MA.DTYPES.values())[i % 3] for i in range(k)]


def _model(mode, hp, seed=0):
    lr, wd, mom, damp, nest = hp
    rng = np.random.RandomState(seed)
    dts = _dtypes(mode, len(LENS))
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(m).astype(np.float32)).to(dt))
              for m, dt in zip(LENS, dts)]
    groups = [{"params": [p], "name": f"p{i}", "lr": lr, "weight_decay": wd, "momentum": mom, "dampening": damp,
               "nesterov": nest} for i, p in enumerate(params)]
    return params, groups, list(enumerate(g["name"] for g in groups)), dts, rng


@pytest.mark.parametrize("entry", ["loop", "apply_gradient"])
@pytest.mark.parametrize("name", sorted(HPS))
@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp32", "mixed"])
def test_cpu_master_loop_matches_the_model(mode, name, entry):
    """Three steps: master, fp32 buffers and parameters after every step.  CPU tensors take the
    loop through utils.apply_gradient(master=...) as well."""
    from chocosgd_amd import utils
    hp = HPS[name]
    params, groups, names, dts, rng = _model(mode, hp)
    mw = utils.MasterWeights(groups, names)
    assert mw.buffer.dtype == torch.float32
    assert same_bits(mw.buffer.numpy(), np.concatenate([MA.host(p) for p in params])), "the pack widens exactly"
    state = collections.defaultdict(dict)
    masters = [MA.host(p) for p in params]
    bufs = [None] * len(params)
    for k in range(STEPS):
        for p in params:
            p.grad = torch.from_numpy((0.1 * rng.standard_normal(p.numel())).astype(np.float32)).to(p.dtype)
        grads = [MA.host(p.grad) for p in params]
        if entry == "loop":
            utils.apply_gradient_master_loop(groups, state, mw)
        else:
            utils.apply_gradient(groups, state, master=mw)
        want_p = []
        for i, dt in enumerate(dts):
            masters[i], bufs[i], pg = MA.master_step(masters[i], grads[i], bufs[i], *hp, first=k == 0,
                                                     dtype=MA.NAMES[dt])
            want_p.append(pg)
        assert same_bits(mw.buffer.numpy(), np.concatenate(masters)), f"master after step {k}"
        for i, p in enumerate(params):
            assert same_bits(MA.host(p), want_p[i]), f"param {i} after step {k}"
            assert same_bits(MA.host(p.grad), grads[i]), "the grads were written"
            if hp[2] != 0:
                buf = state[p]["momentum_buffer"]
                assert buf.dtype == torch.float32 and same_bits(buf.numpy(), bufs[i]), f"buf {i}, step {k}"
            else:
                assert "momentum_buffer" not in state[p]


@pytest.mark.parametrize("name", ["plain", "wd", "mom", "nesterov", "damp"])
def test_fp32_fixtures_replayed_through_the_master_loop(name):
    """With fp32 parameter tensors the master loop is apply_gradient: the reference's own
    recorded parameters and buffers."""
    from chocosgd_amd import utils
    inputs, fx = golden("sgd_inputs"), golden(f"sgd_{name}_apply")
    lr, wd, mom, damp, nest = fx["hp"].tolist()
    lens = inputs["lens"].tolist()
    params, o = [], 0
    for m in lens:
        params.append(torch.nn.Parameter(torch.from_numpy(inputs["p0"][o:o + m].copy())))
        o += m
    groups = [{"params": [p], "name": f"p{i}", "lr": lr, "weight_decay": wd, "momentum": mom, "dampening": damp,
               "nesterov": bool(nest)} for i, p in enumerate(params)]
    mw = utils.MasterWeights(groups, list(enumerate(g["name"] for g in groups)))
    state = collections.defaultdict(dict)
    for k in range(STEPS):
        o = 0
        for p, m in zip(params, lens):
            p.grad = torch.from_numpy(inputs[f"g{k}"][o:o + m].copy())
            o += m
        utils.apply_gradient_master_loop(groups, state, mw)
        assert same_bits(mw.buffer.numpy(), fx[f"p{k}"]), f"master after step {k}"
        assert same_bits(np.concatenate([MA.host(p) for p in params]), fx[f"p{k}"]), f"p after step {k}"
        if mom != 0:
            got = np.concatenate([state[p]["momentum_buffer"].numpy() for p in params])
            assert same_bits(got, fx[f"buf{k}"]), f"buf after step {k}"


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_cpu_lost_updates(name):
    MA.check_lost_updates(name, "cpu", same_bits)


# ----------------------------------------------------------------------------- the master object, refusals
def test_master_weights_round_trip_and_state_dict():
    from chocosgd_amd import utils
    params, groups, names, _, rng = _model("mixed", HPS["plain"])
    mw = utils.MasterWeights(groups, names)
    mw.buffer.copy_(torch.from_numpy(rng.standard_normal(mw.buffer.numel()).astype(np.float32)))
    saved = {k: v.clone() for k, v in mw.state_dict().items()}
    for p in params:
        p.data.mul_(2.0)
    mw.from_model(groups)
    assert same_bits(mw.buffer.numpy(), np.concatenate([MA.host(p) for p in params]))
    mw.load_state_dict(saved)
    assert same_bits(mw.buffer.numpy(), saved["master"].numpy())
    mw.to_model(groups)
    o = 0
    for p, dt in zip(params, _dtypes("mixed", len(params))):
        want = SO.to_grid(saved["master"].numpy()[o:o + p.numel()], MA.NAMES[dt])
        assert same_bits(MA.host(p), want), "to_model is the narrowing of the master"
        o += p.numel()
    assert mw.spare.shape == mw.buffer.shape and mw.spare.data_ptr() != mw.buffer.data_ptr()
    a, b = mw.buffer.data_ptr(), mw.spare.data_ptr()
    mw.swap()
    assert (mw.buffer.data_ptr(), mw.spare.data_ptr()) == (b, a)
    with pytest.raises(RuntimeError):
        mw.load_state_dict({"master": torch.zeros(3)})


def test_cpu_refusals_change_nothing():
    from chocosgd_amd import utils
    params, groups, names, _, rng = _model("bf16", HPS["mom"])
    for p in params:
        p.grad = torch.ones_like(p)
    mw = utils.MasterWeights(groups, names)
    state = collections.defaultdict(dict)

    def snapshot():
        return [mw.buffer.clone()] + [p.detach().clone() for p in params]

    def unchanged(snap):
        return all(torch.equal(a, b) for a, b in zip(snap, snapshot()))

    snap = snapshot()
    with pytest.raises(RuntimeError):
        utils.apply_gradient(groups, state, apply_grad_to_model=False, master=mw)
    with pytest.raises(RuntimeError):
        utils.apply_gradient(groups, state, flat_out=torch.zeros(mw.buffer.numel()), master=mw)
    with pytest.raises(RuntimeError):
        utils.fused_step(None, groups, names, None, None, None, 0.9, 0, master=mw)
    state[params[3]]["momentum_buffer"] = torch.zeros_like(params[3])  # a bf16 buffer of the 16-bit step
    with pytest.raises(RuntimeError, match="float32 momentum buffers"):
        utils.apply_gradient(groups, state, master=mw)
    with pytest.raises(RuntimeError, match="float32 momentum buffers"):
        utils.apply_gradient_master_loop(groups, state, mw)
    del state[params[3]]["momentum_buffer"]
    other = utils.MasterWeights(groups[:-1], names[:-1])  # built for another (smaller) model
    with pytest.raises(RuntimeError):
        utils.apply_gradient(groups, state, master=other)
    assert unchanged(snap) and all("momentum_buffer" not in state[p] for p in params)
