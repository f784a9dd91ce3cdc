"""Stochastic rounding for bf16 models, host side (no GPU): the restatement of the rounding and
of its bit stream (chocosgd_amd/rounding.py, written from include/choco_codec.h), the argument
checks of choco_params_unpack_sr / choco_params_sgd_sr (made before any HIP call), the host-side
counter, the refused combinations, and the accumulation experiment that motivates the feature."""
import collections
import ctypes

import numpy as np
import pytest
import torch

from chocosgd_amd import _lib, codec, utils
from chocosgd_amd.tensor_buffer import TensorBuffer

ERR_INVALID = -1  # CHOCO_ERR_INVALID
F32, BF16, F16 = 0, 1, 2
GRAD, WRITE_PARAMS, WRITE_GRADS, ADD_FLAT, WRITE_CLIPPED = 1, 2, 4, 8, 16
ALL_R16 = np.arange(65536, dtype=np.uint16)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def _narrow_all(value):
    """sr_narrow_bf16 of one fp32 value with every r16: 65536 bf16 bit patterns (uint16)."""
    x = torch.full((65536,), float(value), dtype=torch.float32)
    if np.isnan(value):
        x = torch.from_numpy(np.full(65536, value, dtype=np.float32))
    out = utils.sr_narrow_bf16(x, ALL_R16)
    assert out.dtype == torch.bfloat16 and out.shape == x.shape
    return out.view(torch.int16).numpy().view(np.uint16)


# a handful of inputs off the bf16 grid: ordinary, negative, just below a binade boundary (the
# successor is the next binade's first value), a subnormal, the largest finite fp32
OFF_GRID = [0x3F804000, 0xBF80C001, 0x3FFFFFFF, 0x40490FDB, 0xC2F6E979, 0x00012345, 0x807FFFFF, 0x7F7FFFFF,
            0x3F800001, 0x3F80FFFF]


@pytest.mark.parametrize("bits", OFF_GRID)
def test_narrow_is_truncation_or_successor_with_exact_counts(bits):
    got = _narrow_all(_f32(bits))
    trunc, low = bits >> 16, bits & 0xFFFF
    assert set(np.unique(got).tolist()) == {trunc, trunc + 1}
    assert int((got == trunc + 1).sum()) == low  # P(successor) = low16 / 65536, exactly
    # the successor is taken exactly by the r16 that carry
    assert np.array_equal(got == trunc + 1, ALL_R16.astype(np.uint32) + low >= 65536)
    if bits == 0x3FFFFFFF:
        assert trunc + 1 == 0x4000  # across the binade boundary: 2.0
    if bits == 0x7F7FFFFF:
        assert trunc + 1 == 0x7F80  # past the largest finite bf16: inf, as rounding up does
    if bits == 0x807FFFFF:
        assert trunc + 1 == 0x8080  # the largest subnormal's successor: the smallest normal, negative


@pytest.mark.parametrize("bits", [0x00000000, 0x80000000, 0x3F800000, 0xBF810000, 0x7F7F0000, 0x00010000, 0x80400000,
                                  0x7F800000, 0xFF800000])
def test_values_on_the_bf16_grid_never_move(bits):
    got = _narrow_all(_f32(bits))
    assert np.all(got == bits >> 16)  # +-0, +-inf, bf16 subnormals, the largest finite bf16 included


def test_nan_becomes_the_quiet_nan():
    for bits in [0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x7FFF8000]:
        assert np.all(_narrow_all(_f32(bits)) == 0x7FC0)


def test_narrow_keeps_shape_and_checks_its_arguments():
    x = torch.randn(3, 5)
    out = utils.sr_narrow_bf16(x, np.zeros(15, dtype=np.uint16))
    assert out.shape == x.shape
    # r16 = 0 truncates: toward zero in magnitude
    assert np.array_equal(out.view(torch.int16).numpy().view(np.uint16),
                          (x.numpy().view(np.uint32) >> 16).astype(np.uint16))
    with pytest.raises(RuntimeError):
        utils.sr_narrow_bf16(x.double(), np.zeros(15, dtype=np.uint16))
    with pytest.raises(RuntimeError):
        utils.sr_narrow_bf16(x, np.zeros(14, dtype=np.uint16))


def _mix(z):
    """SplitMix64's output function in Python integers: the header's definition, a second time."""
    m = (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_bits_follow_the_header_definition():
    m = (1 << 64) - 1
    for seed, step in [(0, 0), (5, 3), (2 ** 64 - 1, 2 ** 40 + 7)]:
        key = _mix((seed + (step + 1) * 0xD1B54A32D192ED03) & m)
        got = utils.sr_bits(seed, step, 0, 41)
        assert got.dtype == np.uint16
        for i in range(41):
            w = _mix((key + ((i >> 2) + 1) * 0x9E3779B97F4A7C15) & m)
            assert int(got[i]) == (w >> (16 * (i & 3))) & 0xFFFF, (seed, step, i)


def test_bits_do_not_depend_on_start():
    whole = utils.sr_bits(5, 3, 0, 10_000)
    for start, n in [(0, 1), (1, 7), (3, 8190), (8191, 9), (4093, 5000), (9999, 1), (17, 0)]:
        assert np.array_equal(utils.sr_bits(5, 3, start, n), whole[start:start + n]), (start, n)
    far = utils.sr_bits(5, 3, 2 ** 31 - 5, 5)  # the end of the largest layout
    assert far.shape == (5,) and np.array_equal(far[1:], utils.sr_bits(5, 3, 2 ** 31 - 4, 4))


def test_streams_of_other_steps_and_seeds_differ():
    base = utils.sr_bits(5, 3, 0, 4096)
    for seed, step in [(5, 4), (6, 3), (5, 2), (0, 3)]:
        other = utils.sr_bits(seed, step, 0, 4096)
        # independent 16-bit draws agree in about 4096 / 65536 places
        assert int((other == base).sum()) <= 4, (seed, step)


def test_bits_are_uniform_over_the_top_four():
    draws = utils.sr_bits(11, 0, 0, 1 << 20)
    counts = np.bincount(draws >> 12, minlength=16)
    sigma = np.sqrt((1 << 20) * (1 / 16) * (15 / 16))  # about 248
    assert counts.sum() == 1 << 20
    assert np.all(np.abs(counts - 65536) <= 6 * sigma), counts


# ----------------------------------------------------------------------------- the ABI, without a device
def _unpack_call(lib, ptrs, lens, dts, n, flat=0x10000, nseg=None, null=()):
    k = len(ptrs)
    a_p = (ctypes.c_void_p * max(k, 1))(*ptrs)
    a_l = (ctypes.c_int64 * max(k, 1))(*lens)
    a_d = (ctypes.c_int32 * max(k, 1))(*dts)
    args = [None if "ptrs" in null else a_p, None if "lens" in null else a_l, None if "dtypes" in null else a_d]
    return lib.choco_params_unpack_sr(*args, k if nseg is None else nseg, ctypes.c_void_p(flat), n, 5, 3, None)


UNPACK_BAD = {
    "fp16 tensor": dict(ptrs=[0x1000, 0x2000], lens=[4, 4], dts=[BF16, F16], n=8, msg="tensor 1: fp16"),
    "null ptrs": dict(ptrs=[0x1000], lens=[4], dts=[BF16], n=4, null=("ptrs",), msg="null table"),
    "null lens": dict(ptrs=[0x1000], lens=[4], dts=[BF16], n=4, null=("lens",), msg="null table"),
    "null dtypes": dict(ptrs=[0x1000], lens=[4], dts=[BF16], n=4, null=("dtypes",), msg="null table"),
    "null tensor": dict(ptrs=[0x1000, 0], lens=[4, 4], dts=[BF16, F32], n=8, msg="null pointer"),
    "null flat": dict(ptrs=[0x1000], lens=[4], dts=[BF16], n=4, flat=0, msg="null flat"),
    "sum below n": dict(ptrs=[0x1000, 0x2000], lens=[4, 4], dts=[F32, BF16], n=9, msg="add up"),
    "sum above n": dict(ptrs=[0x1000, 0x2000], lens=[4, 4], dts=[F32, BF16], n=7, msg="add up"),
    "bf16 at odd byte": dict(ptrs=[0x1001], lens=[4], dts=[BF16], n=4, msg="aligned"),
    "nseg zero": dict(ptrs=[0x1000], lens=[4], dts=[BF16], n=4, nseg=0, msg="nseg"),
    "nseg negative": dict(ptrs=[0x1000], lens=[4], dts=[BF16], n=4, nseg=-2, msg="nseg"),
}


@pytest.mark.parametrize("case", sorted(UNPACK_BAD))
def test_unpack_sr_rejects_invalid_arguments(lib, case):
    kw = dict(UNPACK_BAD[case])
    msg = kw.pop("msg")
    before = codec.launch_count("param_unpack_sr_kernel")
    assert _unpack_call(lib, **kw) == ERR_INVALID, case
    err = _lib.last_error()
    assert msg in err, (case, err)
    assert codec.launch_count("param_unpack_sr_kernel") == before  # nothing was launched


def _sgd_call(lib, dts=(BF16, F32), lens=(4, 4), n=8, mode=WRITE_PARAMS, flat=0x10000, coef=None, nseg=None,
              null=(), grads=(0x3000, 0x4000), flags=(0, 0)):
    k = len(dts)
    vp = lambda vals: (ctypes.c_void_p * k)(*vals)  # noqa: E731
    f64 = lambda v: (ctypes.c_double * k)(*([v] * k))  # noqa: E731
    tables = {"params": vp([0x1000, 0x2000][:k]), "grads": vp(list(grads)[:k]), "bufs": vp([0] * k),
              "lens": (ctypes.c_int64 * k)(*lens), "dtypes": (ctypes.c_int32 * k)(*dts), "lr": f64(0.1), "wd": f64(0.0),
              "mom": f64(0.0), "damp": f64(0.0), "flags": (ctypes.c_int32 * k)(*flags)}
    args = [None if name in null else t for name, t in tables.items()]
    return lib.choco_params_sgd_sr(*args, k if nseg is None else nseg, ctypes.c_void_p(flat), n, mode,
                                   None if coef is None else ctypes.c_void_p(coef), 5, 3, None)


SGD_BAD = {
    "fp16 tensor": dict(dts=(BF16, F16), msg="tensor 1: fp16"),
    "grad mode": dict(mode=GRAD | WRITE_GRADS, msg="apply mode"),
    "grad mode, no write": dict(mode=GRAD, msg="apply mode"),
    "add_flat": dict(mode=GRAD | WRITE_GRADS | ADD_FLAT, msg="apply mode"),
    "add_flat alone": dict(mode=WRITE_PARAMS | ADD_FLAT, msg="ADD_FLAT"),
    "write_clipped without coef": dict(mode=WRITE_PARAMS | WRITE_CLIPPED, msg="unknown mode bits"),
    "unknown mode bit": dict(mode=WRITE_PARAMS | 32, msg="unknown mode bits"),
    "misaligned coef": dict(coef=0x5002, msg="coef"),
    "null params": dict(null=("params",), msg="null table"),
    "null lens": dict(null=("lens",), msg="null table"),
    "null lr": dict(null=("lr",), msg="null table"),
    "null grad": dict(grads=(0x3000, 0), msg="null grad"),
    "nothing to write": dict(mode=0, flat=0, msg="nothing to write"),
    "sum below n": dict(n=9, msg="add up"),
    "sum above n": dict(n=7, msg="add up"),
    "nseg zero": dict(nseg=0, msg="nseg"),
    "nseg negative": dict(nseg=-1, msg="nseg"),
}


@pytest.mark.parametrize("case", sorted(SGD_BAD))
def test_sgd_sr_rejects_invalid_arguments(lib, case):
    kw = dict(SGD_BAD[case])
    msg = kw.pop("msg")
    before = codec.launch_count("param_sgd_sr_kernel")
    assert _sgd_call(lib, **kw) == ERR_INVALID, case
    err = _lib.last_error()
    assert msg in err, (case, err)
    assert codec.launch_count("param_sgd_sr_kernel") == before  # nothing was launched


def test_existing_entry_points_and_version_are_unchanged(lib):
    assert lib.choco_version() == 1
    assert lib.choco_params_launches(0) == 0 and lib.choco_params_sgd_launches(-1) == 0


# ----------------------------------------------------------------------------- the counter
def test_counter_advances_by_one_per_next():
    sr = utils.StochasticRounding(seed=7)
    assert [sr.next() for _ in range(3)] == [(7, 0), (7, 1), (7, 2)]
    assert sr.state_dict() == {"seed": 7, "step": 3}


def test_state_dict_round_trip_continues_the_stream():
    a = utils.StochasticRounding(seed=2 ** 63 + 11)
    for _ in range(5):
        a.next()
    b = utils.StochasticRounding(seed=0)
    b.load_state_dict(a.state_dict())
    assert all(isinstance(v, int) for v in a.state_dict().values()) and len(a.state_dict()) == 2
    assert [b.next() for _ in range(3)] == [a.next() for _ in range(3)]
    x = torch.randn(100)
    pa, pb = a.next(), b.next()
    assert torch.equal(utils.sr_narrow_bf16(x, utils.sr_bits(*pa, 0, 100)).view(torch.int16),
                       utils.sr_narrow_bf16(x, utils.sr_bits(*pb, 0, 100)).view(torch.int16))


def _model(dtypes, n=16, lr=0.5):
    params = [torch.nn.Parameter(torch.ones(n, dtype=dt)) for dt in dtypes]
    for p in params:
        p.grad = torch.ones_like(p.data)
    groups = [{"params": [p], "name": f"p{i}", "lr": lr, "weight_decay": 0.0, "momentum": 0.0, "dampening": 0.0,
               "nesterov": False} for i, p in enumerate(params)]
    return params, groups, list(enumerate(g["name"] for g in groups))


def test_refused_combinations_raise_and_leave_the_stream_alone():
    params, groups, names = _model([torch.bfloat16, torch.float32])
    state = collections.defaultdict(dict)
    sr = utils.StochasticRounding(3)
    master = utils.MasterWeights(groups, names)
    scaler = utils.LossScaler("cpu")
    with pytest.raises(RuntimeError, match="master"):
        utils.apply_gradient(groups, state, master=master, rounding=sr)
    with pytest.raises(RuntimeError, match="loss"):
        utils.apply_gradient(groups, state, loss_scale=scaler, rounding=sr)
    with pytest.raises(RuntimeError, match="apply_grad_to_model"):
        utils.apply_gradient(groups, state, apply_grad_to_model=False, rounding=sr)
    fused = dict(compressor=None, param_groups=groups, param_names=names, shapes=None, neighbor_hat_params=None,
                 neighbors_info=None, consensus_stepsize=0.5, rank=0)
    with pytest.raises(RuntimeError, match="state"):
        utils.fused_step(**fused, rounding=sr)
    with pytest.raises(RuntimeError, match="master"):
        utils.fused_step(**fused, state=state, master=master, rounding=sr)
    with pytest.raises(RuntimeError, match="loss"):
        utils.fused_step(**fused, state=state, loss_scale=scaler, rounding=sr)
    p16, g16, _ = _model([torch.float16])
    with pytest.raises(RuntimeError, match="float16"):
        utils.apply_gradient(g16, state, rounding=sr)
    with pytest.raises(RuntimeError, match="float16"):
        TensorBuffer([p.data.float() for p in p16]).unpack([p.data for p in p16], rounding=sr)
    assert sr.state_dict()["step"] == 0  # refused before the stream advanced
    assert all(torch.equal(p.data, torch.ones_like(p.data)) for p in params + p16)  # nothing was stepped


def test_steps_outside_the_feature_refuse_rounding():
    from chocosgd_amd import dcd, deep_squeeze, dgc, ecd, ef_sign
    sr = utils.StochasticRounding(3)
    calls = [(utils.dpsgd_step, 5), (utils.allreduce_sgd_step, 4), (dcd.fused_step, 7), (ecd.fused_step, 8),
             (deep_squeeze.fused_step, 7), (ef_sign.fused_step, 5), (dgc.fused_step, 6)]
    for fn, nargs in calls:
        with pytest.raises(RuntimeError, match="rounding"):
            fn(*([None] * nargs), rounding=sr)
    assert sr.state_dict()["step"] == 0


# ----------------------------------------------------------------------------- the loop on CPU tensors
def test_cpu_apply_gradient_takes_the_loop_and_matches_the_restatement():
    params, groups, _ = _model([torch.bfloat16, torch.float32, torch.bfloat16], n=37, lr=2.0 ** -10)
    g = torch.Generator().manual_seed(1)
    for p in params:
        p.data.copy_(torch.randn(37, generator=g))
        p.grad = torch.randn(37, generator=g).to(p.dtype)
    params[2].grad = None
    before = [p.data.clone() for p in params]
    flat = torch.empty(3 * 37)
    utils.apply_gradient(groups, collections.defaultdict(dict), flat_out=flat, rounding=(9, 4))
    new0 = before[0].float().add(params[0].grad.float(), alpha=-2.0 ** -10)
    assert torch.equal(flat[:37], new0)  # unrounded
    assert torch.equal(params[0].data.view(torch.int16),
                       utils.sr_narrow_bf16(new0, utils.sr_bits(9, 4, 0, 37)).view(torch.int16))
    assert torch.equal(params[1].data, before[1].add(params[1].grad, alpha=-2.0 ** -10))  # fp32: as without
    assert torch.equal(flat[37:74], params[1].data)
    assert torch.equal(params[2].data, before[2]) and torch.equal(flat[74:], before[2].float())  # no grad: packed
    # the unpack rounds a flat buffer the same way, at the tensors' flat offsets
    outs = [torch.zeros_like(p.data) for p in params]
    TensorBuffer.from_flat(flat, [p.shape for p in params]).unpack(outs, rounding=(9, 4))
    assert torch.equal(outs[0].view(torch.int16), params[0].data.view(torch.int16))
    assert torch.equal(outs[1], params[1].data)
    assert torch.equal(outs[2].view(torch.int16),
                       utils.sr_narrow_bf16(flat[74:], utils.sr_bits(9, 4, 74, 37)).view(torch.int16))


@pytest.mark.parametrize("seed", [0, 5, 99])
def test_small_updates_survive_in_expectation(seed):
    """4096 bf16 parameters at 1.0, g = 1.0, lr = 2^-12 (a sixteenth of the bf16 ulp below 1.0,
    2^-8), 256 steps.  Round to nearest loses every step.  Stochastic rounding: each step moves a
    parameter down one ulp with probability 1/16, so the mean is near 1 - 256 * 2^-12 = 0.9375;
    per element sigma ~ 2^-8 * sqrt(256 / 16) = 0.0156, over 4096 elements 2.4e-4, and the bound is
    6 sigma.  (Measured with this stream: 0.93726, 0.93722, 0.93771 for seeds 0, 5, 99.)"""
    n, steps, lr = 4096, 256, 2.0 ** -12
    params, groups, _ = _model([torch.bfloat16], n=n, lr=lr)
    state = collections.defaultdict(dict)
    for _ in range(steps):
        utils.apply_gradient_loop(groups, state)
    assert torch.equal(params[0].data, torch.ones(n, dtype=torch.bfloat16))  # every update was lost

    sr = utils.StochasticRounding(seed)
    for _ in range(steps):
        utils.apply_gradient_sr_loop(groups, state, *sr.next())
    assert sr.state_dict()["step"] == steps
    mean = float(params[0].data.double().mean())
    print(f"seed {seed}: mean {mean:.5f}")
    assert abs(mean - 0.9375) <= 1.5e-3, mean
