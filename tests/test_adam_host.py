"""The Adam / AdamW update, host side (no GPU): the numpy restatement (tests/_adam_oracle.py)
against torch's per-tensor CPU optimizer -- the only place torch is the yardstick --,
utils.apply_adam on CPU tensors against the restatement bit for bit, the state's round trip
through torch.optim.AdamW, the refusals, the launch count rule and the argument checks of
choco_params_adam / choco_params_adam_master, made before any HIP call."""
import collections
import copy
import ctypes

import numpy as np
import pytest
import torch

from conftest import same_bits
import _adam_oracle as AO
import _sgd_oracle as SO

ERR_INVALID = -1  # CHOCO_ERR_INVALID
F32, BF16, F16 = 0, 1, 2
DECOUPLED, FIRST, NOGRAD = 1, 2, 4
WRITE_PARAMS, WRITE_CLIPPED = 2, 16
STEPS, N, LR = 20, 4099, 1e-3
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}

# (optimizer, weight decay, beta1): AdamW's decoupled decay, Adam's coupled one, beta1 0.4 for the
# second branch of torch's lerp (weight 1 - beta1 >= 0.5), and no decay at all
CONFIGS = {"adamw": ("AdamW", 0.01, 0.9), "adam": ("Adam", 1e-4, 0.9), "adamw-b0.4": ("AdamW", 0.01, 0.4),
           "adam-b0.4": ("Adam", 1e-4, 0.4), "adam-nowd": ("Adam", 0.0, 0.9)}


@pytest.fixture(scope="module")
def lib():
    from chocosgd_amd import _lib
    return _lib.load()


def _inputs(dtype, seed):
    rng = np.random.RandomState(seed)
    p0 = SO.to_grid((rng.standard_normal(N) * 10.0 ** rng.uniform(-2, 0, N)).astype(np.float32), dtype)
    grads = [SO.to_grid((rng.standard_normal(N) * 10.0 ** rng.uniform(-3, 0, N)).astype(np.float32), dtype)
             for _ in range(STEPS)]
    return p0, grads


def _torch_run(kind, wd, beta1, p0, grads, tdt):
    """torch's per-tensor CPU optimizer on one tensor of dtype tdt; returns (p, exp_avg, exp_avg_sq)."""
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(tdt))
    opt = getattr(torch.optim, kind)([p], lr=LR, betas=(beta1, 0.999), eps=1e-8, weight_decay=wd, foreach=False,
                                     fused=False)
    for g in grads:
        p.grad = torch.from_numpy(g.copy()).to(tdt)
        opt.step()
    f = lambda t: t.detach().to(torch.float64).numpy() if tdt == torch.float64 else t.detach().float().numpy()  # noqa: E731
    return f(p), f(opt.state[p]["exp_avg"]), f(opt.state[p]["exp_avg_sq"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_restatement_against_torch(name, dtype):
    """20 steps on 4099 elements: the restatement is as close to the float64 optimizer as
    torch's own CPU kernel of the same dtype is.  The unit is max(|p_truth|, lr) * 2^-23 (2^-7
    for bf16); the mean error may exceed torch's by 5 %, the max by a factor of 3 (both sides
    are correctly rounded op sequences that differ in where addcdiv rounds, and a max over 4099
    elements is an extreme value).  Where the weight decay is decoupled or zero the moments
    never see p, and equal torch's bit for bit.

    Observed (mean ratio, max ratio) with this file's seeds, fp32: adam 1.0105, 1.160;
    adam-b0.4 0.9921, 1.157; adam-nowd 1.0001, 0.925; adamw 1.0000, 1.000; adamw-b0.4 1.0005,
    0.864.  bf16, all five: 1.0000, 1.000 -- the narrowing to bf16 after addcdiv hides the
    rounding position."""
    kind, wd, beta1 = CONFIGS[name]
    p0, grads = _inputs(dtype, 11 + sorted(CONFIGS).index(name))
    truth, _, _ = _torch_run(kind, wd, beta1, p0, grads, torch.float64)
    tp, tm, tv = _torch_run(kind, wd, beta1, p0, grads, TDT[dtype])
    p, m, v = p0, None, None
    for k, g in enumerate(grads):
        p, m, v, _ = AO.adam_step(p, g, m, v, LR, beta1, 0.999, 1e-8, wd, k + 1, decoupled=kind == "AdamW",
                                  first=k == 0, dtype=dtype)
    unit = np.maximum(np.abs(truth), LR) * 2.0 ** (-23 if dtype == "fp32" else -7)
    err_o, err_t = np.abs(p.astype(np.float64) - truth) / unit, np.abs(tp.astype(np.float64) - truth) / unit
    mean_ratio, max_ratio = err_o.mean() / err_t.mean(), err_o.max() / err_t.max()
    print(f"{dtype} {name}: mean {err_o.mean():.4f} vs torch {err_t.mean():.4f} (ratio {mean_ratio:.4f}), "
          f"max {err_o.max():.3f} vs torch {err_t.max():.3f} (ratio {max_ratio:.3f})")
    assert mean_ratio <= 1.05 and max_ratio <= 3.0
    if kind == "AdamW" or wd == 0:
        assert same_bits(m, tm) and same_bits(v, tv)


# ----------------------------------------------------------------------------- apply_adam on CPU tensors
LENS = [5, 4099, 1, 33, 260, 20011]  # the last one long enough for torch to hand its CPU sqrt to a vector library


def _cpu_model(dtype=torch.float32, nograd=(2,), seed=3):
    rng = np.random.RandomState(seed)
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(m).astype(np.float32)).to(dtype)) for m in LENS]
    groups = []
    for i, p in enumerate(params):
        groups.append({"params": [p], "lr": 1e-3 * (1 + i), "betas": (0.4 if i == 1 else 0.9, 0.999), "eps": 1e-8,
                       "weight_decay": 0.0 if i == 3 else 0.01, "decoupled_weight_decay": i % 2 == 0,
                       "amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
                       "differentiable": False, "fused": None})
    return params, groups


def _set_grads(params, step, nograd=(2,)):
    rng = np.random.RandomState(100 + step)
    for i, p in enumerate(params):
        g = torch.from_numpy((0.1 * rng.standard_normal(p.numel())).astype(np.float32)).to(p.dtype)
        p.grad = None if i in nograd else g


def _np(t):
    return t.detach().float().numpy().copy()


@pytest.mark.parametrize("with_flat", [False, True])
def test_cpu_apply_adam_is_the_restatement(with_flat):
    from chocosgd_amd import utils
    params, groups = _cpu_model()
    state = collections.defaultdict(dict)
    flat = torch.full((sum(LENS),), -7.0) if with_flat else None
    want = [(_np(p), None, None) for p in params]
    for k in range(3):
        _set_grads(params, k)
        grads = [None if p.grad is None else _np(p.grad) for p in params]
        utils.apply_adam(groups, state, flat_out=flat)
        for i, (p, gr) in enumerate(zip(params, groups)):
            if grads[i] is None:
                assert p not in state and same_bits(_np(p), want[i][0])
                continue
            pw, mw, vw = want[i]
            want[i] = AO.adam_step(pw, grads[i], mw, vw, gr["lr"], gr["betas"][0], gr["betas"][1], gr["eps"],
                                   gr["weight_decay"], k + 1, gr["decoupled_weight_decay"], first=k == 0)[:3]
            assert same_bits(_np(p), want[i][0]), (k, i, "p")
            assert same_bits(_np(state[p]["exp_avg"]), want[i][1]), (k, i, "exp_avg")
            assert same_bits(_np(state[p]["exp_avg_sq"]), want[i][2]), (k, i, "exp_avg_sq")
            assert same_bits(_np(p.grad), grads[i]), "the gradient was written"
            step = state[p]["step"]
            assert step.dtype == torch.float32 and step.dim() == 0 and not step.is_cuda and float(step) == k + 1
        if with_flat:
            assert same_bits(flat.numpy(), np.concatenate([w[0] for w in want]))


def test_cpu_apply_adam_with_master_weights_follows_the_fp32_model():
    """A bf16 model with master weights against the fp32 model on the widened gradients: the
    master is the fp32 trajectory, the parameters are its narrowing, the moments are fp32."""
    from chocosgd_amd import utils
    p16, g16 = _cpu_model(torch.bfloat16, nograd=())
    p32, g32 = _cpu_model(torch.float32, nograd=())
    for a, b in zip(p16, p32):
        b.data.copy_(a.data.float())
    names = [(i, f"p{i}") for i in range(len(LENS))]
    mw = utils.MasterWeights(g16, names)
    s16, s32 = collections.defaultdict(dict), collections.defaultdict(dict)
    for k in range(3):
        _set_grads(p16, k, nograd=())
        for a, b in zip(p16, p32):
            b.grad = a.grad.float()
        utils.apply_adam(g16, s16, master=mw, clip_norm=0.5)
        utils.apply_adam(g32, s32, clip_norm=0.5)
        want = np.concatenate([_np(p) for p in p32])
        assert same_bits(mw.buffer.numpy(), want), k
        assert same_bits(np.concatenate([_np(p) for p in p16]), SO.to_grid(want, "bf16")), k
        assert all(s16[p]["exp_avg"].dtype == torch.float32 for p in p16)
        assert all(same_bits(_np(s16[a]["exp_avg_sq"]), _np(s32[b]["exp_avg_sq"])) for a, b in zip(p16, p32))


def test_state_loads_into_torch_adamw_and_back():
    """Three steps here, the state handed to torch.optim.AdamW through its own load_state_dict,
    a step there; and the other way round, with the moments and the count taken over as they
    are."""
    from chocosgd_amd import utils
    params = [torch.nn.Parameter(torch.randn(m, generator=torch.Generator().manual_seed(m))) for m in (7, 130)]
    opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=0.01, foreach=False, fused=False)
    state = collections.defaultdict(dict)
    for k in range(3):
        for p in params:
            p.grad = torch.full_like(p, 0.01 * (k + 1))
        utils.apply_adam(opt.param_groups, state)
    sd = opt.state_dict()
    sd["state"] = {i: {key: val.clone() for key, val in state[p].items()} for i, p in enumerate(params)}
    opt.load_state_dict(sd)
    for i, p in enumerate(params):
        assert float(opt.state[p]["step"]) == 3 and torch.equal(opt.state[p]["exp_avg"], state[p]["exp_avg"])
    opt.step()
    assert all(float(opt.state[p]["step"]) == 4 for p in params)
    # and back: torch's state is apply_adam's, key for key
    before = [(_np(p), _np(opt.state[p]["exp_avg"]), _np(opt.state[p]["exp_avg_sq"])) for p in params]
    utils.apply_adam(opt.param_groups, opt.state)
    for p, (p4, m4, v4) in zip(params, before):
        assert float(opt.state[p]["step"]) == 5
        want = AO.adam_step(p4, _np(p.grad), m4, v4, 1e-3, wd=0.01, step=5, decoupled=True)
        assert same_bits(_np(p), want[0]) and same_bits(_np(opt.state[p]["exp_avg"]), want[1])
        assert same_bits(_np(opt.state[p]["exp_avg_sq"]), want[2]) and not same_bits(want[0], p4)
    fresh = torch.optim.AdamW(params, lr=1e-3, weight_decay=0.01, foreach=False, fused=False)
    fresh.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert all(float(fresh.state[p]["step"]) == 5 for p in params)


# ----------------------------------------------------------------------------- refusals
def _snapshot(params, state):
    return [(p.detach().clone(), None if p.grad is None else p.grad.clone(),
             {k: v.clone() for k, v in state.get(p, {}).items()}) for p in params]


def _unchanged(params, state, snap):
    for p, (p0, g0, st0) in zip(params, snap):
        assert torch.equal(p.detach(), p0) and (g0 is None or torch.equal(p.grad, g0))
        assert set(state.get(p, {})) == set(st0)
        for k, v in st0.items():
            assert torch.equal(state[p][k], v), k


REFUSED = {
    "amsgrad": dict(group={"amsgrad": True}),
    "maximize": dict(group={"maximize": True}),
    "capturable": dict(group={"capturable": True}),
    "differentiable": dict(group={"differentiable": True}),
    "tensor lr": dict(group={"lr": torch.tensor(1e-3)}),
    "tensor beta": dict(group={"betas": (torch.tensor(0.9), 0.999)}),
    "write_clipped without clip_norm": dict(kw={"write_clipped": True}),
    "total_norm without clip_norm": dict(kw={"total_norm": 1.0}),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
@pytest.mark.parametrize("warm", [False, True])
def test_refusals_raise_before_anything_changes(case, warm):
    """The refused key sits in the LAST group: nothing of the groups before it may have moved."""
    from chocosgd_amd import utils
    params, groups = _cpu_model()
    state = collections.defaultdict(dict)
    _set_grads(params, 0)
    if warm:
        utils.apply_adam(groups, state)
    groups[-1].update(REFUSED[case].get("group", {}))
    snap = _snapshot(params, state)
    with pytest.raises(RuntimeError):
        utils.apply_adam(groups, state, **REFUSED[case].get("kw", {}))
    _unchanged(params, state, snap)
    with pytest.raises(RuntimeError):
        utils.apply_adam_loop(groups, state, **REFUSED[case].get("kw", {}))
    _unchanged(params, state, snap)


def test_master_refuses_moments_of_another_dtype_and_flat_out():
    from chocosgd_amd import utils
    params, groups = _cpu_model(torch.bfloat16, nograd=())
    names = [(i, f"p{i}") for i in range(len(LENS))]
    state = collections.defaultdict(dict)
    _set_grads(params, 0, nograd=())
    utils.apply_adam(groups, state)  # bf16 moments
    mw = utils.MasterWeights(groups, names)
    snap = _snapshot(params, state)
    before = mw.buffer.clone()
    with pytest.raises(RuntimeError, match="float32 moments"):
        utils.apply_adam(groups, state, master=mw)
    with pytest.raises(RuntimeError, match="flat_out"):
        utils.apply_adam(groups, collections.defaultdict(dict), master=mw, flat_out=torch.zeros(sum(LENS)))
    _unchanged(params, state, snap)
    assert torch.equal(mw.buffer, before)
    # fp32 moments beside 16-bit parameters need the master copy
    state32 = collections.defaultdict(dict)
    utils.apply_adam(groups, state32, master=mw)
    snap = _snapshot(params, state32)
    with pytest.raises(RuntimeError, match="master copy"):
        utils.apply_adam(groups, state32)
    _unchanged(params, state32, snap)


def test_fused_step_refuses_what_has_no_adam_form():
    from chocosgd_amd import utils
    params, groups = _cpu_model(nograd=())
    names = [(i, f"p{i}") for i in range(len(LENS))]
    _set_grads(params, 0, nograd=())
    state = collections.defaultdict(dict)
    snap = _snapshot(params, state)
    args = (None, groups, names, None, None, None, 0.5, 0)
    with pytest.raises(RuntimeError, match="section 8"):
        utils.fused_step(*args, state=state, update="adam", loss_scale=utils.LossScaler("cpu"))
    with pytest.raises(RuntimeError, match="section 8"):
        utils.fused_step(*args, state=state, update="adam", rounding=(1, 2))
    with pytest.raises(RuntimeError, match="state"):
        utils.fused_step(*args, update="adam")
    with pytest.raises(RuntimeError, match="update"):
        utils.fused_step(*args, state=state, update="lamb")
    groups[-1]["amsgrad"] = True
    with pytest.raises(RuntimeError, match="amsgrad"):
        utils.fused_step(*args, state=state, update="adam")
    _unchanged(params, state, snap)


# ----------------------------------------------------------------------------- the C ABI
def test_launches_rule(lib):
    from chocosgd_amd import codec
    cap = max(k for k in range(1, 1024) if lib.choco_params_adam_launches(k) == 1)
    assert cap == 54  # four pointers a tensor: below the SGD table's 72
    for nseg in [1, cap - 1, cap, cap + 1, 3000]:
        assert lib.choco_params_adam_launches(nseg) == -(-nseg // cap), nseg
        assert codec.params_adam_launches(nseg) == -(-nseg // cap)
    assert lib.choco_params_adam_launches(161) == 3  # ResNet-50
    assert lib.choco_params_adam_launches(0) == 0 and lib.choco_params_adam_launches(-4) == 0


TABLES = ["params", "grads", "exp_avg", "exp_avg_sq", "lens", "dtypes", "lr", "beta1", "beta2", "eps", "wd", "step", "flags"]


def _call(lib, p, g, m, v, lens, dts, n, lr=None, beta1=None, beta2=None, eps=None, wd=None, step=None, flags=None,
          flat=0x10000, mode=WRITE_PARAMS, coef=0, nseg=None, null=(), master=False, msg=None):
    """One call with host tables built from the lists; the made-up device pointers are never
    dereferenced (every case here is rejected before the first launch)."""
    k = len(p)
    arr = lambda ct, vals: (ct * max(k, 1))(*vals)  # noqa: E731
    dbl = lambda vals, d: arr(ctypes.c_double, vals or [d] * k)  # noqa: E731
    tabs = [arr(ctypes.c_void_p, p), arr(ctypes.c_void_p, g), arr(ctypes.c_void_p, m), arr(ctypes.c_void_p, v),
            arr(ctypes.c_int64, lens), arr(ctypes.c_int32, dts), dbl(lr, 1e-3), dbl(beta1, 0.9), dbl(beta2, 0.999),
            dbl(eps, 1e-8), dbl(wd, 0.0), dbl(step, 1.0), arr(ctypes.c_int32, flags or [0] * k)]
    a = [None if nm in null else t for nm, t in zip(TABLES, tabs)]
    fn = lib.choco_params_adam_master if master else lib.choco_params_adam
    return fn(*a, k if nseg is None else nseg, ctypes.c_void_p(flat), n, mode, ctypes.c_void_p(coef), None)


ONE = dict(p=[0x1000], g=[0x2000], m=[0x3000], v=[0x4000], lens=[4], dts=[F32], n=4)
TWO = dict(p=[0x1000, 0x1100], g=[0x2000, 0x2100], m=[0x3000, 0x3100], v=[0x4000, 0x4100], lens=[4, 4], dts=[F32, BF16],
           n=8)
BAD = {
    **{f"null {t}": dict(ONE, null=(t,), msg="null table") for t in TABLES},
    "nseg zero": dict(ONE, nseg=0, msg="nseg"),
    "n = 2^31": dict(ONE, lens=[2 ** 31], n=2 ** 31, msg="2^31"),
    "unknown mode bit": dict(ONE, mode=1 | WRITE_PARAMS, msg="mode"),
    "write_clipped without coef": dict(ONE, mode=WRITE_PARAMS | WRITE_CLIPPED, msg="WRITE_CLIPPED needs coef"),
    "nothing to write": dict(ONE, flat=0, mode=0, msg="nothing to write"),
    "master null": dict(ONE, flat=0, master=True, msg="master is null"),
    "flat at 2 mod 4": dict(ONE, flat=0x10002, msg="4-byte"),
    "coef at 2 mod 4": dict(ONE, coef=0x5002, msg="coef"),
    "negative length": dict(TWO, lens=[-4, 8], n=4, msg="negative length"),
    "dtype 3": dict(ONE, dts=[3], msg="dtype"),
    "sum above n": dict(TWO, n=7, msg="add up"),
    "sum below n": dict(TWO, n=9, msg="add up"),
    "unknown flag bit": dict(ONE, flags=[8], msg="flag"),
    "fp32 param at 2 mod 4": dict(ONE, p=[0x1002], msg="aligned"),
    "bf16 grad at odd byte": dict(TWO, g=[0x2000, 0x2101], msg="aligned"),
    "bf16 exp_avg at odd byte": dict(TWO, m=[0x3000, 0x3101], msg="aligned"),
    "master: bf16 tensor's exp_avg_sq at 2 mod 4": dict(TWO, v=[0x4000, 0x4102], master=True, msg="aligned"),
    "null param": dict(TWO, p=[0x1000, 0], msg="null param"),
    "null param of a no-grad tensor": dict(TWO, p=[0x1000, 0], flags=[0, NOGRAD], msg="null param"),
    "null grad": dict(TWO, g=[0, 0x2100], msg="null grad"),
    "null exp_avg": dict(TWO, m=[0x3000, 0], msg="null exp_avg"),
    "null exp_avg_sq, FIRST (written all the same)": dict(TWO, v=[0x4000, 0], flags=[0, FIRST], msg="null exp_avg"),
    "negative lr": dict(ONE, lr=[-1e-3], msg="lr"),
    "beta1 = 1": dict(ONE, beta1=[1.0], msg="betas"),
    "beta2 negative": dict(ONE, beta2=[-0.1], msg="betas"),
    "beta1 nan": dict(ONE, beta1=[float("nan")], msg="betas"),
    "eps negative": dict(ONE, eps=[-1e-8], msg="eps"),
    "weight decay negative": dict(ONE, wd=[-0.1], msg="weight_decay"),
    "step zero": dict(ONE, step=[0.0], msg="step"),
    # the first failing check in layout_check's order is the one reported
    "order: nseg before the mode bits": dict(ONE, nseg=0, mode=1, msg="nseg"),
    "order: mode bits before a tensor's dtype": dict(ONE, mode=1, dts=[3], msg="mode"),
    "order: coef alignment before a tensor's pointers": dict(ONE, coef=0x5002, p=[0], msg="coef"),
    "order: tensor 0's null grad before tensor 1's dtype": dict(TWO, g=[0, 0x2100], dts=[F32, 7], msg="null grad"),
    "order: dtype before the same tensor's flags": dict(ONE, dts=[3], flags=[8], msg="dtype"),
    "order: flags before alignment": dict(ONE, flags=[8], p=[0x1002], msg="flag"),
    "order: alignment before null": dict(TWO, p=[0, 0x1100], g=[0x2000, 0x2101], lens=[0, 4], n=4, msg="aligned"),
    "order: null moment before the betas": dict(ONE, m=[0], beta1=[2.0], msg="null exp_avg"),
    "order: betas before eps before step": dict(ONE, beta1=[2.0], eps=[-1.0], step=[0.0], msg="betas"),
    "order: eps before step": dict(ONE, eps=[-1.0], step=[0.0], msg="eps"),
    "order: step before the sum": dict(ONE, step=[0.0], n=5, msg="step"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_arguments_are_rejected(lib, case):
    from chocosgd_amd import _lib
    assert _call(lib, **BAD[case]) == ERR_INVALID, case
    err = _lib.last_error()
    assert err != "" and BAD[case]["msg"] in err, (case, err)


def test_no_grad_and_zero_length_tensors_need_no_pointers(lib):
    """What the checks let through is seen by a call that fails on a LATER check: a zero-length
    tensor with null pointers and a no-grad tensor with null grad and moments pass theirs."""
    from chocosgd_amd import _lib
    rc = _call(lib, p=[0, 0x1100, 0x1200], g=[0, 0, 0x2200], m=[0, 0, 0x3200], v=[0, 0, 0x4200], lens=[0, 4, 4],
               dts=[F32, F16, BF16], flags=[0, NOGRAD, DECOUPLED | FIRST], step=[1.0, 1.0, 0.0], n=8)
    assert rc == ERR_INVALID and "tensor 2: step" in _lib.last_error()
