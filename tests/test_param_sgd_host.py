"""apply_gradient, host side (no GPU): the numpy oracle and utils.apply_gradient's per-tensor
loop against the reference's fixtures (tests/golden/sgd_*.npz, gen_golden_sgd.py), bit for bit;
the launch count rule; the argument checks of choco_params_sgd, made before any HIP call."""
import collections
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import golden, same_bits
import _sgd_oracle as SO

CAP = 72  # tensors per launch (sgd.hip kSgdCap)
ERR_INVALID = -1  # CHOCO_ERR_INVALID
F32, BF16, F16 = 0, 1, 2
NESTEROV, FIRST, NOGRAD = 1, 2, 4
APPLY, GRAD, WRITE_PARAMS, WRITE_GRADS = 0, 1, 2, 4
SETS = ["plain", "wd", "mom", "nesterov", "damp"]
MODES = ["apply", "grad"]
STEPS = 3


@pytest.fixture(scope="module")
def lib():
    from chocosgd_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def inputs():
    return golden("sgd_inputs")


def _hp(fx):
    lr, wd, mom, damp, nest = fx["hp"].tolist()
    return lr, wd, mom, damp, bool(nest)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SETS)
def test_oracle_matches_the_reference_fixtures(inputs, name, mode):
    fx = golden(f"sgd_{name}_{mode}")
    lr, wd, mom, damp, nest = _hp(fx)
    p, buf = inputs["p0"], None
    for k in range(STEPS):
        p_new, buf, d = SO.sgd_step(p, inputs[f"g{k}"], buf, lr, wd, mom, damp, nest, first=k == 0)
        if mode == "apply":
            p = p_new
        assert same_bits(p, fx[f"p{k}"]), f"p after step {k}"
        if mom != 0:
            assert same_bits(buf, fx[f"buf{k}"]), f"buf after step {k}"
        if f"d{k}" in fx:
            assert same_bits(d, fx[f"d{k}"]), f"d_p after step {k}"


def _fma_exact(a, b, c):
    """a * b + c in rational arithmetic, rounded once to fp32 (nearest, ties to even)."""
    q = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if q == 0:
        return np.float32(0.0)
    e = abs(q.numerator).bit_length() - q.denominator.bit_length()
    e -= 1 if abs(q) < Fraction(2) ** e else 0      # 2^e <= |q| < 2^(e+1)
    ulp = Fraction(2) ** (max(e, -126) - 23)
    return np.float32(float(round(q / ulp) * ulp))  # round(): half to even; the product is exact


def test_oracle_fma_rounds_once():
    # 2^-24 (1 + 2^-23) * (1 - 2^-23) = 2^-24 - 2^-70: with c = 1 + 2^-23 the exact sum lies just
    # below a tie of fp32; a float64 sum drops the 2^-70, lands ON the tie and rounds to even, up
    a, b, c = np.float32(2.0 ** -24 * (1 + 2.0 ** -23)), np.float32(1 - 2.0 ** -23), np.float32(1 + 2.0 ** -23)
    naive = np.float32(np.float64(a) * np.float64(b) + np.float64(c))
    assert naive == np.float32(1 + 2.0 ** -22) and _fma_exact(a, b, c) == c
    assert SO.fma32(a, b, c) == c
    rng = np.random.RandomState(1)
    n = 3000
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    c = (a.astype(np.float64) * b * 2.0 ** rng.randint(-30, 30, n)).astype(np.float32)
    # a product near half an ulp of c, and results in the subnormal range
    c[:500] = (np.abs(a[:500].astype(np.float64) * b[:500]) * 2.0 ** 24).astype(np.float32)
    a[500:600] *= np.float32(2.0 ** -70)
    b[500:600] *= np.float32(2.0 ** -70)
    c[500:600] *= np.float32(2.0 ** -140)
    got = SO.fma32(a, b, c)
    want = np.array([_fma_exact(x, y, z) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert np.array_equal(got, want)


def _cpu_model(inputs, hp, dtype=torch.float32):
    lr, wd, mom, damp, nest = hp
    lens = inputs["lens"].tolist()
    params, o = [], 0
    for m in lens:
        params.append(torch.nn.Parameter(torch.from_numpy(inputs["p0"][o:o + m].copy()).to(dtype)))
        o += m
    groups = [{"params": [p], "lr": lr, "weight_decay": wd, "momentum": mom, "dampening": damp, "nesterov": nest}
              for p in params]
    return params, groups, lens


def _set_grads(params, flat, lens):
    o = 0
    for p, m in zip(params, lens):
        p.grad = torch.from_numpy(flat[o:o + m].copy()).to(p.dtype)
        o += m


def _cat(tensors):
    return np.concatenate([t.detach().float().numpy().reshape(-1) for t in tensors])


@pytest.mark.parametrize("with_flat", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SETS)
def test_cpu_apply_gradient_matches_the_reference_fixtures(inputs, name, mode, with_flat):
    from chocosgd_amd import utils
    fx = golden(f"sgd_{name}_{mode}")
    hp = _hp(fx)
    params, groups, lens = _cpu_model(inputs, hp)
    state = collections.defaultdict(dict)
    flat = torch.full((sum(lens),), -7.0) if with_flat else None
    for k in range(STEPS):
        _set_grads(params, inputs[f"g{k}"], lens)
        grads = [p.grad for p in params]
        utils.apply_gradient(groups, state, apply_grad_to_model=mode == "apply", flat_out=flat)
        assert same_bits(_cat(params), fx[f"p{k}"]), f"p after step {k}"
        if hp[2] != 0:
            assert same_bits(_cat([state[p]["momentum_buffer"] for p in params]), fx[f"buf{k}"]), f"buf, step {k}"
        assert all(p.grad is g for p, g in zip(params, grads)), "p.grad must not be rebound"
        if mode == "grad":
            assert same_bits(_cat(grads), fx[f"d{k}"]), f"d_p after step {k}"
            if with_flat:
                assert same_bits(flat.numpy(), fx[f"d{k}"]), f"flat d_p after step {k}"
        else:
            assert same_bits(_cat(grads), inputs[f"g{k}"]), "apply mode must not write the grads"
            if with_flat:
                assert same_bits(flat.numpy(), fx[f"p{k}"]), f"flat p after step {k}"


def test_cpu_apply_gradient_skips_what_the_reference_skips():
    """p.grad is None: untouched, no state entry; momentum 0: no buffer is created."""
    from chocosgd_amd import utils
    a, b = torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2))
    a.grad = torch.full((3,), 0.5)
    groups = [{"params": [a, b], "lr": 0.1, "weight_decay": 0.0, "momentum": 0.0, "dampening": 0.0,
               "nesterov": False}]
    state = collections.defaultdict(dict)
    flat = torch.zeros(5)
    utils.apply_gradient(groups, state, flat_out=flat)
    assert torch.equal(a.data, torch.full((3,), 1 - np.float32(0.1) * np.float32(0.5)))
    assert torch.equal(b.data, torch.ones(2)) and b.grad is None
    assert "momentum_buffer" not in state[a] and b not in state
    assert torch.equal(flat, torch.cat([a.data, b.data]))


def test_launches_rule(lib):
    from chocosgd_amd import codec
    for nseg in [1, CAP - 1, CAP, CAP + 1, 3000]:
        assert lib.choco_params_sgd_launches(nseg) == -(-nseg // CAP), nseg
        assert codec.params_sgd_launches(nseg) == -(-nseg // CAP)
    assert lib.choco_params_sgd_launches(161) == 3  # ResNet-50: three launches, not 161 x 5
    assert lib.choco_params_sgd_launches(0) == 0 and lib.choco_params_sgd_launches(-4) == 0


def _call(lib, p, g, b, lens, dts, n, lr=None, wd=None, mom=None, damp=None, flags=None, flat=0x10000, mode=WRITE_PARAMS,
          nseg=None, null=(), msg=None):
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
    return lib.choco_params_sgd(*a, k if nseg is None else nseg, ctypes.c_void_p(flat), n, mode, None)


ONE = dict(p=[0x1000], g=[0x2000], b=[0x3000], lens=[4], dts=[F32], n=4)
TWO = dict(p=[0x1000, 0x1100], g=[0x2000, 0x2100], b=[0x3000, 0x3100], lens=[4, 4], dts=[F32, BF16], n=8)
BAD = {
    **{f"null {t}": dict(ONE, null=(t,), msg="null table")
       for t in ["params", "grads", "bufs", "lens", "dtypes", "lr", "wd", "mom", "damp", "flags"]},
    "nseg zero": dict(ONE, nseg=0, msg="nseg"),
    "nseg negative": dict(ONE, nseg=-3, msg="nseg"),
    "negative length": dict(TWO, lens=[-4, 8], n=4, msg="negative length"),
    "sum below n": dict(TWO, n=9, msg="add up"),
    "sum above n": dict(TWO, n=7, msg="add up"),
    "n = 2^31": dict(ONE, lens=[2 ** 31], n=2 ** 31, msg="2^31"),
    "dtype 3": dict(ONE, dts=[3], msg="dtype"),
    "dtype -1": dict(ONE, dts=[-1], msg="dtype"),
    "fp32 param at 2 mod 4": dict(ONE, p=[0x1002], msg="aligned"),
    "fp32 grad at 2 mod 4": dict(ONE, g=[0x2002], msg="aligned"),
    "fp32 buf at 2 mod 4": dict(ONE, b=[0x3002], mom=[0.9], msg="aligned"),
    "bf16 grad at odd byte": dict(TWO, g=[0x2000, 0x2101], msg="aligned"),
    "fp16 buf at odd byte": dict(TWO, dts=[F32, F16], b=[0x3000, 0x3101], msg="aligned"),
    "flat at 2 mod 4": dict(ONE, flat=0x10002, msg="4-byte"),
    "null param": dict(TWO, p=[0x1000, 0], msg="null param"),
    "null param of a no-grad tensor": dict(TWO, p=[0x1000, 0], flags=[0, NOGRAD], msg="null param"),
    "null grad": dict(TWO, g=[0, 0x2100], msg="null grad"),
    "null buf with momentum": dict(TWO, b=[0x3000, 0], mom=[0.9, 0.9], msg="null momentum buffer"),
    "nesterov without momentum": dict(ONE, flags=[NESTEROV], mom=[0.0], msg="nesterov"),
    "nesterov with negative momentum": dict(ONE, flags=[NESTEROV], mom=[-0.5], msg="nesterov"),
    "nesterov with dampening": dict(ONE, flags=[NESTEROV], mom=[0.9], damp=[0.1], msg="nesterov"),
    "no-grad tensor in grad mode": dict(TWO, flags=[0, NOGRAD], mode=GRAD | WRITE_GRADS, msg="no-grad"),
    "apply, nothing to write": dict(ONE, flat=0, mode=APPLY, msg="nothing to write"),
    "grad, nothing to write": dict(ONE, flat=0, mode=GRAD, msg="nothing to write"),
    "grad mode writing params": dict(ONE, mode=GRAD | WRITE_PARAMS, msg="grad mode"),
    "apply mode writing grads": dict(ONE, mode=APPLY | WRITE_GRADS, msg="apply mode"),
    "unknown mode bit": dict(ONE, mode=8 | WRITE_PARAMS, msg="mode"),
    "unknown flag bit": dict(ONE, flags=[8], msg="flag"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_arguments_are_rejected(lib, case):
    from chocosgd_amd import _lib
    assert _call(lib, **BAD[case]) == ERR_INVALID, case
    err = _lib.last_error()
    assert err != "" and BAD[case]["msg"] in err, (case, err)
