"""Dynamic loss scaling, host side (no GPU): the numpy model's state machine (_lscale_oracle)
against torch._amp_update_scale_; utils.apply_gradient(loss_scale=) on CPU tensors (the loop
path) against the model, bit for bit at the total the loop measured, skipped steps included;
its fp32 agreement with torch's own unscale + clip + update at a power-of-two scale; LossScaler's
checkpoint; the keyword errors; and the argument checks of choco_params_gradnorm_scaled,
choco_params_sgd_scaled and choco_params_sgd_master_scaled, made before any HIP call.

The total alone has a tolerance, test_gpu_gclip's: equal or adjacent on the coefficient dtype's
grid to the fp64 value (the order of an fp64 sum of n < 2^31 squares moves it by far less than
half an fp32 ulp)."""
import collections
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden, same_bits
import _gclip_oracle as GO
import _lscale_oracle as LO
import _sgd_oracle as SO

ERR_INVALID, ERR_WORKSPACE = -1, -3
F32, BF16, F16 = 0, 1, 2
NOGRAD = 4
APPLY, GRAD, WRITE_PARAMS, WRITE_GRADS, ADD_FLAT, WRITE_CLIPPED = 0, 1, 2, 4, 8, 16
TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SCALES = {"fp32": 1000.0, "bf16": 1000.0, "fp16": 100.0}  # not powers of two: 1 / scale is rounded


@pytest.fixture(scope="module")
def lib():
    from chocosgd_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def inputs():
    return golden("gclip_inputs")


def _split(flat, lens):
    offs = np.concatenate([[0], np.cumsum(lens)])
    return [flat[offs[i]:offs[i + 1]] for i in range(len(lens))]


def _cat(tensors):
    return np.concatenate([t.detach().float().numpy().reshape(-1) for t in tensors])


# ------------------------------------------------------------------ the state machine against torch
@pytest.mark.parametrize("interval", [1, 2, 3])
@pytest.mark.parametrize("growth,backoff", [(2.0, 0.5), (1.7, 0.3)])
def test_state_machine_matches_amp_update_scale(growth, backoff, interval):
    script = [0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    scale, tracker = torch.tensor([1000.0]), torch.zeros(1, dtype=torch.int32)
    s, t = np.float32(1000.0), 0
    grew = backed_off = False
    for f in script:
        before = s
        torch._amp_update_scale_(scale, tracker, torch.tensor([float(f)]), growth, backoff, interval)
        s, t = LO.update(s, t, bool(f), growth, backoff, interval)
        assert same_bits(scale.numpy(), [s]) and int(tracker) == t, (f, scale, s, tracker, t)
        grew, backed_off = grew or s > before, backed_off or s < before
    assert grew and backed_off, "the script must back off and grow"


def test_state_machine_growth_past_fp32_is_not_applied():
    top = float(2.0 ** 127)
    scale, tracker = torch.tensor([top]), torch.tensor([1], dtype=torch.int32)
    torch._amp_update_scale_(scale, tracker, torch.zeros(1), 2.0, 0.5, 2)
    assert LO.update(top, 1, False, 2.0, 0.5, 2) == (np.float32(top), 0)
    assert float(scale) == top and int(tracker) == 0


# ------------------------------------------------------------------ the loop path against the model
def _cpu_model(inputs, hp, dtype):
    lr, wd, mom, damp, nest = hp
    lens = inputs["lens"].tolist()
    params = [torch.nn.Parameter(torch.from_numpy(v.copy()).to(TORCH_DT[dtype]))
              for v in _split(SO.to_grid(inputs["p0"], dtype), lens)]
    groups = [{"params": [p], "name": f"p{i}", "lr": lr, "weight_decay": wd, "momentum": mom, "dampening": damp,
               "nesterov": nest} for i, p in enumerate(params)]
    return params, groups, lens


def _set_grads(params, flat, lens, dtype):
    for p, v in zip(params, _split(flat, lens)):
        p.grad = torch.from_numpy(v.copy()).to(TORCH_DT[dtype])


def _check_out(last, raw_split, scale, max_norm, cd):
    """The step's four floats against the model: the total within 1 ulp of CD's grid (an
    overflowed one: the same non-finite value), the rest bit for bit at that total."""
    is_found = LO.found(raw_split)
    want = LO.total(raw_split, scale, cd)
    if np.isfinite(want):
        assert same_bits(last[:1], SO.to_grid(last[:1], cd)) and GO.ulp_distance(last[0], want, cd) <= 1, (last, want)
    else:
        assert same_bits(last[:1], [want])
    assert same_bits(last, LO.out(last[0], max_norm, scale, is_found, cd)), (last, scale, is_found)
    return is_found


@pytest.mark.parametrize("max_norm", [None, 0.4])
@pytest.mark.parametrize("master", [False, True], ids=["plain", "master"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_cpu_loop_matches_the_model(inputs, dtype, master, max_norm):
    """Steps: overflow (a first step: no buffer may be left), taken, overflow, taken, taken.
    fp32 and master: the update is _sgd_oracle's.  A 16-bit model without master: torch's CPU ops
    round a Python scalar (lr, weight decay, momentum) to the tensor's dtype, which the kernel's
    model (fp32 scalars) does not, so there the parameters are compared with
    utils.apply_gradient_loop on a twin model given the oracle's unscaled gradients -- what the
    loop path is defined as; everything loss scaling adds is still the oracle's, bit for bit."""
    from chocosgd_amd import utils
    hp = (0.1, 1e-4, 0.9, 0.1, False)
    params, groups, lens = _cpu_model(inputs, hp, dtype)
    mw = utils.MasterWeights(groups, [(i, g["name"]) for i, g in enumerate(groups)]) if master else None
    scaler = utils.LossScaler("cpu", init_scale=SCALES[dtype], growth_interval=2)
    state = collections.defaultdict(dict)
    math_dt = "fp32" if master else dtype
    cd = "fp32" if master else dtype
    p, buf = SO.to_grid(inputs["p0"], dtype), None
    twin = None if master or dtype == "fp32" else _cpu_model(inputs, hp, dtype)
    twin_state = collections.defaultdict(dict)
    scale, tracker = np.float32(SCALES[dtype]), 0
    bad = {0: np.inf, 2: np.nan}
    seen_growth = False
    for k in range(5):
        raw = SO.to_grid(SO.mul32(inputs[f"g{k % 3}"], scale), dtype)
        if k in bad:
            raw[lens[0] + 3] = bad[k]
        _set_grads(params, raw, lens, dtype)
        utils.apply_gradient(groups, state, master=mw, clip_norm=max_norm, write_clipped=True, loss_scale=scaler)
        last = scaler.last.numpy()
        is_found = _check_out(last, _split(raw, lens), scale, max_norm, cd)
        assert is_found == (k in bad) == scaler.skipped()
        if is_found:
            assert same_bits(_cat([q.grad for q in params]), raw), "a skipped step wrote the gradients"
            if buf is None:
                assert all("momentum_buffer" not in state[q] for q in params), "a skipped first step left buffers"
        else:
            gu = LO.unscale(raw, last[1], math_dt)
            if twin is None:
                p, buf, _ = SO.sgd_step(p, gu, buf, *hp, first=buf is None, dtype=math_dt)
            else:
                _set_grads(twin[0], gu, lens, dtype)
                utils.apply_gradient_loop(twin[1], twin_state)
                p, buf = _cat(twin[0]), _cat([twin_state[q]["momentum_buffer"] for q in twin[0]])
            assert same_bits(_cat([q.grad for q in params]), SO.to_grid(gu, dtype)), "write_clipped"
        new_scale, tracker = LO.update(scale, tracker, is_found, interval=2)
        seen_growth |= bool(new_scale > scale)
        scale = new_scale
        assert same_bits(scaler._scale.numpy(), [scale]) and int(scaler._growth_tracker) == tracker
        if master:
            assert same_bits(mw.buffer.numpy(), p), f"master after step {k}"
        assert same_bits(_cat(params), SO.to_grid(p, dtype)), f"params after step {k}"
        if buf is not None:
            assert same_bits(_cat([state[q]["momentum_buffer"] for q in params]), buf), f"buf after step {k}"
    assert seen_growth and scaler.get_scale() == float(scale)


def test_cpu_loop_without_write_clipped_leaves_the_gradients_and_fills_flat(inputs):
    from chocosgd_amd import utils
    hp = (0.1, 0.0, 0.0, 0.0, False)
    params, groups, lens = _cpu_model(inputs, hp, "fp32")
    scaler = utils.LossScaler("cpu", init_scale=1000.0)
    raw = SO.mul32(inputs["g0"], np.float32(1000.0))
    _set_grads(params, raw, lens, "fp32")
    flat = torch.zeros(sum(lens))
    utils.apply_gradient(groups, collections.defaultdict(dict), flat_out=flat, loss_scale=scaler)
    want, _, _ = SO.sgd_step(inputs["p0"], LO.unscale(raw, scaler.last.numpy()[1]), None, *hp)
    assert same_bits(_cat(params), want) and same_bits(flat.numpy(), want)
    assert same_bits(_cat([q.grad for q in params]), raw)
    raw[5] = -np.inf
    _set_grads(params, raw, lens, "fp32")
    utils.apply_gradient(groups, collections.defaultdict(dict), flat_out=flat, loss_scale=scaler)
    assert scaler.skipped() and same_bits(_cat(params), want) and same_bits(flat.numpy(), want)
    assert scaler.get_scale() == 500.0


# ------------------------------------------------------------------ fp32: torch's own unscale, clip and update
@pytest.mark.parametrize("hp", [(0.1, 0.0, 0.0, 0.0, False), (0.1, 5e-4, 0.9, 0.0, True), (0.1, 1e-4, 0.9, 0.1, False)],
                         ids=["plain", "nesterov", "damp"])
def test_fp32_loop_equals_torchs_unscale_then_clip_then_update(inputs, hp):
    """With a power-of-two scale and gradients away from the fp32 subnormals, multiplying by
    1 / scale is exact, so g * (c * inv) == (g * inv) * c and the loss-scaled step equals
    _amp_foreach_non_finite_check_and_unscale_, clip_grad_norm_loop and apply_gradient_loop at
    the same total, bit for bit."""
    from chocosgd_amd import utils
    scale = 4096.0
    a, ga, lens = _cpu_model(inputs, hp, "fp32")
    b, gb, _ = _cpu_model(inputs, hp, "fp32")
    sa, sb = collections.defaultdict(dict), collections.defaultdict(dict)
    scaler = utils.LossScaler("cpu", init_scale=scale)
    clipped = []
    for k in range(3):
        raw = SO.mul32(inputs[f"g{k}"], np.float32(scale))
        assert np.all((raw == 0) | (np.abs(raw) > 1e-30))
        _set_grads(a, raw, lens, "fp32")
        _set_grads(b, raw, lens, "fp32")
        utils.apply_gradient(ga, sa, clip_norm=0.4, write_clipped=True, loss_scale=scaler)
        found = torch.zeros(1)
        torch._amp_foreach_non_finite_check_and_unscale_([q.grad for q in b], found, torch.tensor(1.0 / scale))
        assert float(found) == 0.0
        utils.clip_grad_norm_loop(b, 0.4, total_norm=scaler.last[0])
        clipped.append(float(scaler.last[1]) < 1.0 / scale)
        utils.apply_gradient_loop(gb, sb)
        assert same_bits(_cat(a), _cat(b)), f"params after step {k}"
        assert same_bits(_cat([q.grad for q in a]), _cat([q.grad for q in b])), f"clipped gradients, step {k}"
        if hp[2] != 0:
            assert same_bits(_cat([sa[q]["momentum_buffer"] for q in a]), _cat([sb[q]["momentum_buffer"] for q in b]))
    assert clipped == [True, True, False], "the fixture's gradients: clipped in steps 0 and 1, not in step 2"


# ------------------------------------------------------------------ LossScaler
def test_loss_scaler_state_dict_round_trip_and_torch_checkpoint():
    from chocosgd_amd import utils
    a = utils.LossScaler("cpu", init_scale=512.0, growth_factor=1.7, backoff_factor=0.3, growth_interval=7)
    a._growth_tracker.fill_(5)
    sd = a.state_dict()
    assert set(sd) == {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}
    b = utils.LossScaler("cpu")
    assert b.get_scale() == 65536.0 and b.growth_interval == 2000 and not b.skipped()
    b.load_state_dict(sd)
    assert b.state_dict() == sd and b.get_scale() == 512.0 and int(b._growth_tracker) == 5
    theirs = torch.amp.GradScaler("cpu", init_scale=128.0, growth_interval=11).state_dict()
    assert set(theirs) == set(sd)
    b.load_state_dict(theirs)
    assert b.get_scale() == 128.0 and b.growth_interval == 11 and b.growth_factor == 2.0 and b.backoff_factor == 0.5
    loss = torch.tensor([3.0, -1.5], dtype=torch.float16)
    scaled = b.scale(loss)
    assert scaled.dtype == torch.float16 and scaled.tolist() == [384.0, -192.0]
    assert b.scale(torch.tensor(2.0)).shape == ()


@pytest.mark.parametrize("kw", [dict(init_scale=0.0), dict(init_scale=-2.0), dict(init_scale=float("inf")),
                                dict(init_scale=float("nan")), dict(init_scale=1e39), dict(growth_factor=1.0),
                                dict(growth_factor=float("inf")), dict(backoff_factor=1.0), dict(backoff_factor=0.0),
                                dict(growth_interval=0), dict(growth_interval=1.5)], ids=str)
def test_loss_scaler_refuses_bad_factors(kw):
    from chocosgd_amd import utils
    with pytest.raises(RuntimeError, match="LossScaler"):
        utils.LossScaler("cpu", **kw)
    ok = utils.LossScaler("cpu")
    sd = dict(ok.state_dict())
    sd.update({"scale" if k == "init_scale" else k: v for k, v in kw.items()})
    with pytest.raises(RuntimeError, match="LossScaler"):
        ok.load_state_dict(sd)
    assert ok.get_scale() == 65536.0


def test_keyword_errors():
    from chocosgd_amd import codec, utils
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.ones(4)
    groups = [{"params": [p], "lr": 0.1, "weight_decay": 0.0, "momentum": 0.0, "dampening": 0.0, "nesterov": False}]
    state = collections.defaultdict(dict)
    scaler = utils.LossScaler("cpu")
    with pytest.raises(RuntimeError, match="grad mode"):
        utils.apply_gradient(groups, state, apply_grad_to_model=False, loss_scale=scaler)
    with pytest.raises(RuntimeError, match="total_norm"):
        utils.apply_gradient(groups, state, clip_norm=1.0, total_norm=1.0, loss_scale=scaler)
    with pytest.raises(RuntimeError, match="LossScaler"):
        utils.apply_gradient(groups, state, loss_scale=65536.0)
    with pytest.raises(RuntimeError, match="state"):
        utils.fused_step(None, groups, [(0, "p")], None, None, None, 0.5, 0, loss_scale=scaler)
    assert torch.equal(p.data, torch.ones(4)) and torch.equal(p.grad, torch.ones(4)) and scaler.last is None
    # ParamSgdPlan refuses scaled together with the other clips before it touches a tensor
    plan = object.__new__(codec.ParamSgdPlan)
    plan.n, plan.nseg, plan.device = 4, 1, torch.device("cpu")
    marker = object()
    for kw in (dict(gclip=marker), dict(norms=marker, clip_threshold=1.0), dict(add_flat=True), dict(grad_mode=True)):
        with pytest.raises(RuntimeError, match="does not combine"):
            plan.run(None, scaled=marker, **kw)


# ------------------------------------------------------------------ the ABI: exported, and checked before any launch
def _arr(ct, vals, k):
    return (ct * max(k, 1))(*vals)


def test_new_functions_are_exported_with_the_old_launch_and_workspace_rules(lib):
    for name in ("choco_params_gradnorm_scaled", "choco_params_sgd_scaled", "choco_params_sgd_master_scaled"):
        assert hasattr(lib, name), name
    assert lib.choco_version() == 1


def _scaled(lib, p, g, b, lens, dts, n, mom=None, flags=None, flat=0x10000, mode=APPLY | WRITE_PARAMS, out=0x20000,
            master=False, msg=None):
    k = len(p)
    a = [_arr(ctypes.c_void_p, p, k), _arr(ctypes.c_void_p, g, k), _arr(ctypes.c_void_p, b, k),
         _arr(ctypes.c_int64, lens, k), _arr(ctypes.c_int32, dts, k), _arr(ctypes.c_double, [0.1] * k, k),
         _arr(ctypes.c_double, [0.0] * k, k), _arr(ctypes.c_double, mom or [0.0] * k, k),
         _arr(ctypes.c_double, [0.0] * k, k), _arr(ctypes.c_int32, flags or [0] * k, k)]
    fn = lib.choco_params_sgd_master_scaled if master else lib.choco_params_sgd_scaled
    return fn(*a, k, ctypes.c_void_p(flat), n, mode, ctypes.c_void_p(out), None)


ONE = dict(p=[0x1000], g=[0x2000], b=[0x3000], lens=[4], dts=[F32], n=4)
TWO = dict(p=[0x1000, 0x1100], g=[0x2000, 0x2100], b=[0x3000, 0x3100], lens=[4, 4], dts=[F32, BF16], n=8)
BAD_SCALED = {
    "null out": dict(ONE, out=0, msg="out"),
    "out at 2 mod 4": dict(ONE, out=0x20002, msg="out"),
    "grad mode": dict(ONE, mode=GRAD | WRITE_GRADS, msg="apply mode"),
    "add_flat": dict(ONE, mode=GRAD | WRITE_GRADS | ADD_FLAT, msg="ADD_FLAT"),
    "unknown mode bit": dict(ONE, mode=32 | WRITE_PARAMS, msg="mode"),
    "apply mode writing grads": dict(ONE, mode=APPLY | WRITE_GRADS, msg="apply mode"),
    "nothing to write": dict(ONE, flat=0, mode=APPLY, msg="nothing to write"),
    "null grad": dict(TWO, g=[0, 0x2100], msg="null grad"),
    "sum below n": dict(TWO, n=9, msg="add up"),
    "master: null out": dict(ONE, master=True, out=0, msg="out"),
    "master: grad mode": dict(ONE, master=True, mode=GRAD, msg="master update"),
    "master: add_flat": dict(ONE, master=True, mode=ADD_FLAT, msg="master update"),
    "master: null master": dict(ONE, master=True, flat=0, msg="master is null"),
    "master: 16-bit momentum buffer": dict(TWO, master=True, b=[0x3000, 0x3102], mom=[0.9, 0.9], msg="aligned"),
}


@pytest.mark.parametrize("case", sorted(BAD_SCALED))
def test_sgd_scaled_invalid_arguments_are_rejected(lib, case):
    from chocosgd_amd import _lib
    assert _scaled(lib, **BAD_SCALED[case]) == ERR_INVALID, case
    err = _lib.last_error()
    assert err != "" and BAD_SCALED[case]["msg"] in err, (case, err)


def _gradnorm(lib, g, lens, dts, n, flags=None, max_norm=0.4, cd=F32, scale=0x22000, tracker=0x22100, growth=2.0,
              backoff=0.5, interval=2000, has_clip=1, out=0x20000, norms=0x21000, ws=0x30000, ws_bytes=1 << 20,
              nseg=None, null=(), msg=None, rc=None):
    k = len(g)
    tabs = {"grads": _arr(ctypes.c_void_p, g, k), "lens": _arr(ctypes.c_int64, lens, k),
            "dtypes": _arr(ctypes.c_int32, dts, k), "flags": _arr(ctypes.c_int32, flags or [0] * k, k)}
    a = [None if nm in null else t for nm, t in tabs.items()]
    return lib.choco_params_gradnorm_scaled(*a, k if nseg is None else nseg, n, max_norm, cd, ctypes.c_void_p(scale),
                                            ctypes.c_void_p(tracker), growth, backoff, interval, has_clip,
                                            ctypes.c_void_p(out), ctypes.c_void_p(norms), ctypes.c_void_p(ws), ws_bytes,
                                            None)


N1 = dict(g=[0x2000], lens=[4], dts=[F32], n=4)
N2 = dict(g=[0x2000, 0x2100], lens=[4, 4], dts=[F32, F16], n=8)
BAD_GRADNORM = {
    **{f"null {t}": dict(N1, null=(t,), msg="null table") for t in ["grads", "lens", "dtypes", "flags"]},
    "nseg zero": dict(N1, nseg=0, msg="nseg"),
    "sum below n": dict(N2, n=9, msg="add up"),
    "fp16 grad at odd byte": dict(N2, g=[0x2000, 0x2101], msg="aligned"),
    "null grad": dict(N2, g=[0, 0x2100], msg="null grad"),
    "max_norm nan": dict(N1, max_norm=float("nan"), msg="max_norm"),
    "max_norm negative": dict(N1, max_norm=-0.5, msg="max_norm"),
    "coef_dtype 3": dict(N1, cd=3, msg="coef_dtype"),
    "null out": dict(N1, out=0, msg="out"),
    "out at 2 mod 4": dict(N1, out=0x20002, msg="out"),
    "null scale_state": dict(N1, scale=0, msg="scale_state"),
    "scale_state at 2 mod 4": dict(N1, scale=0x22002, msg="scale_state"),
    "null growth_tracker": dict(N1, tracker=0, msg="growth_tracker"),
    "growth_tracker at 2 mod 4": dict(N1, tracker=0x22102, msg="growth_tracker"),
    "growth 1": dict(N1, growth=1.0, msg="growth"),
    "growth below 1": dict(N1, growth=0.5, msg="growth"),
    "growth nan": dict(N1, growth=float("nan"), msg="growth"),
    "growth inf": dict(N1, growth=float("inf"), msg="growth"),
    "backoff 1": dict(N1, backoff=1.0, msg="backoff"),
    "backoff 0": dict(N1, backoff=0.0, msg="backoff"),
    "backoff nan": dict(N1, backoff=float("nan"), msg="backoff"),
    "interval 0": dict(N1, interval=0, msg="interval"),
    "has_clip 2": dict(N1, has_clip=2, msg="has_clip"),
    "null workspace": dict(N1, ws=0, msg="workspace"),
    "short workspace": dict(N1, ws_bytes=16, msg="workspace too small", rc=ERR_WORKSPACE),
}


@pytest.mark.parametrize("case", sorted(BAD_GRADNORM))
def test_gradnorm_scaled_invalid_arguments_are_rejected(lib, case):
    from chocosgd_amd import _lib
    assert _gradnorm(lib, **BAD_GRADNORM[case]) == (BAD_GRADNORM[case].get("rc") or ERR_INVALID), case
    err = _lib.last_error()
    assert err != "" and BAD_GRADNORM[case]["msg"] in err, (case, err)
