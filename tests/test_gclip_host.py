"""Global-norm gradient clipping, host side (no GPU): the numpy model (_gclip_oracle) against
torch.nn.utils.clip_grads_with_norm_ and against the reference sequence's fixtures
(tests/golden/gclip_*.npz, gen_golden_gclip.py: clip_grad_norm_ then the reference's
apply_gradient), bit for bit with the fixture's totals pinned; utils.clip_grad_norm_loop and
utils.apply_gradient(clip_norm=) on CPU tensors; the launch-count and workspace rules; the
argument checks of choco_params_gradnorm, choco_params_sgd_gclip and
choco_params_sgd_master_gclip, made before any HIP call."""
import collections
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden, same_bits
import _gclip_oracle as GO
import _sgd_oracle as SO

ERR_INVALID, ERR_WORKSPACE = -1, -3
F32, BF16, F16 = 0, 1, 2
NESTEROV, FIRST, NOGRAD = 1, 2, 4
APPLY, GRAD, WRITE_PARAMS, WRITE_GRADS, ADD_FLAT, WRITE_CLIPPED = 0, 1, 2, 4, 8, 16
SETS = ["clip", "wd", "mom", "nesterov", "damp"]
STEPS = 3
TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module")
def lib():
    from chocosgd_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def inputs():
    return golden("gclip_inputs")


def _hp(fx):
    lr, wd, mom, damp, nest = fx["hp"].tolist()
    return lr, wd, mom, damp, bool(nest)


def _split(flat, lens):
    offs = np.concatenate([[0], np.cumsum(lens)])
    return [flat[offs[i]:offs[i + 1]] for i in range(len(lens))]


# ------------------------------------------------------------------ the model against torch
def _torch_clip(gs, dtypes, total, max_norm, cd):
    """clip_grads_with_norm_ on CPU tensors with the total as a CD tensor; returns fp32 arrays."""
    params = []
    for g, dt in zip(gs, dtypes):
        p = torch.nn.Parameter(torch.zeros(g.size, dtype=TORCH_DT[dt]))
        p.grad = torch.from_numpy(g.copy()).to(TORCH_DT[dt])
        params.append(p)
    torch.nn.utils.clip_grads_with_norm_(params, max_norm, torch.tensor(total, dtype=torch.float32).to(TORCH_DT[cd]))
    return [p.grad.float().numpy() for p in params]


TOTALS = [float("nan"), float("inf"), 0.0, 1.0, 0.4, 0.39999, 3e38, 1e-30, 65504.0, 1e5]
MAX_NORMS = [0.25, 0.4, 1.0, 0.0, 3.0, 1e-3, 1e4]


@pytest.mark.parametrize("dtypes", [["fp32"], ["bf16"], ["fp16"], ["fp32", "bf16", "fp16"], ["bf16", "fp16"]],
                         ids=lambda d: "+".join(d))
def test_model_matches_clip_grads_with_norm(dtypes):
    cd = GO.common_dtype(dtypes)
    rng = np.random.RandomState(7)
    gs = []
    for dt in dtypes:
        g = (rng.standard_normal(257) * 10.0 ** rng.uniform(-3, 2, 257)).astype(np.float32)
        g[:6] = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-41]
        gs.append(SO.to_grid(g, dt))
    rand_t = (10.0 ** rng.uniform(-4, 4, 150)).astype(np.float32).tolist()
    rand_m = (10.0 ** rng.uniform(-3, 2, 150)).tolist()
    pairs = [(t, m) for t in TOTALS for m in MAX_NORMS] + list(zip(rand_t, rand_m))
    seen_clipped = seen_one = False
    for t, m in pairs:
        t = float(SO.to_grid(np.array([t], np.float32), cd)[0])
        c = GO.coef(t, m, cd)
        seen_clipped |= bool(c < 1)
        seen_one |= bool(c == 1)
        want = _torch_clip(gs, dtypes, t, m, cd)
        for g, dt, w in zip(gs, dtypes, want):
            assert same_bits(GO.clip(g, c, dt), w), (t, m, dt, c)
    assert seen_clipped and seen_one


def test_model_special_totals():
    for cd in ["fp32", "bf16", "fp16"]:
        assert np.isnan(GO.coef(np.nan, 0.4, cd))
        assert GO.coef(np.inf, 0.4, cd) == 0 and GO.coef(0.0, 0.4, cd) == 1
        assert GO.coef(1.0, 0.0, cd) == 0
    g = np.array([1.0, -2.0, 0.0, -0.0], np.float32)
    assert same_bits(GO.clip(g, GO.coef(np.inf, 0.4), "fp32"), np.array([0.0, -0.0, 0.0, -0.0], np.float32))
    assert np.all(np.isnan(GO.clip(g, GO.coef(np.nan, 0.4), "fp32")))


def test_one_element_fixture_pins_no_shortcut(inputs):
    """g = 1, max_norm = 1: the total is exactly 1 and the gradient is STILL scaled, by
    (1 / (1 + 1e-6)) * 1 < 1 -- clip_grad_norm_ has no `total >= max_norm` test."""
    assert float(inputs["one_total"]) == 1.0 == float(GO.total([inputs["one_g"]]))
    c = GO.coef(inputs["one_total"], float(inputs["one_max_norm"]))
    assert c < 1
    gc = GO.clip(inputs["one_g"], c)
    assert same_bits(gc, inputs["one_gc"]) and gc[0] != inputs["one_g"][0]
    p, _, _ = SO.sgd_step(inputs["one_p0"], gc, None, float(inputs["one_lr"]))
    assert same_bits(p, inputs["one_p"])


def test_fixture_clips_first_and_not_last(inputs):
    fx = golden("gclip_clip")
    m = float(inputs["max_norm"])
    assert GO.coef(fx["total0"], m) < 1 and GO.coef(fx["total1"], m) < 1 and GO.coef(fx["total2"], m) == 1
    assert not same_bits(fx["gc0"], inputs["g0"]) and same_bits(fx["gc2"], inputs["g2"])


@pytest.mark.parametrize("name", SETS)
def test_model_reproduces_the_reference_fixtures(inputs, name):
    fx = golden(f"gclip_{name}")
    lr, wd, mom, damp, nest = _hp(fx)
    m = float(inputs["max_norm"])
    p, buf = inputs["p0"], None
    for k in range(STEPS):
        gc = GO.clip(inputs[f"g{k}"], GO.coef(fx[f"total{k}"], m))
        assert same_bits(gc, fx[f"gc{k}"]), f"clipped gradient, step {k}"
        p, buf, _ = SO.sgd_step(p, gc, buf, lr, wd, mom, damp, nest, first=k == 0)
        assert same_bits(p, fx[f"p{k}"]), f"params after step {k}"
        if mom != 0:
            assert same_bits(buf, fx[f"buf{k}"]), f"buf after step {k}"


def test_model_total_is_next_to_fp64_and_to_torch(inputs):
    """The model's total is the fp32 rounding of the fp64 value (within 1 ulp however numpy
    orders its fp64 sum), and torch's fp32-accumulated total lies within a few ulp of it."""
    fx = golden("gclip_clip")
    lens = inputs["lens"].tolist()
    for k in range(STEPS):
        g = inputs[f"g{k}"]
        mine = GO.total(_split(g, lens))
        exact = np.float32(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
        assert GO.ulp_distance(mine, exact) <= 1
        assert GO.ulp_distance(mine, fx[f"total{k}"]) <= 8, (mine, fx[f"total{k}"])


# ------------------------------------------------------------------ the CPU paths of utils
def _cpu_model(inputs, hp, dtype=torch.float32):
    lr, wd, mom, damp, nest = hp
    lens = inputs["lens"].tolist()
    params = [torch.nn.Parameter(torch.from_numpy(v.copy()).to(dtype)) for v in _split(inputs["p0"], lens)]
    groups = [{"params": [p], "lr": lr, "weight_decay": wd, "momentum": mom, "dampening": damp, "nesterov": nest}
              for p in params]
    return params, groups, lens


def _set_grads(params, flat, lens, dtype=torch.float32):
    for p, v in zip(params, _split(flat, lens)):
        p.grad = torch.from_numpy(v.copy()).to(dtype)


def _cat(tensors):
    return np.concatenate([t.detach().float().numpy().reshape(-1) for t in tensors])


def test_cpu_clip_grad_norm_loop_matches_the_fixtures(inputs):
    from chocosgd_amd import utils
    fx = golden("gclip_clip")
    params, _, lens = _cpu_model(inputs, _hp(fx))
    for k in range(STEPS):
        _set_grads(params, inputs[f"g{k}"], lens)
        grads = [p.grad for p in params]
        total = utils.clip_grad_norm_loop(params, float(inputs["max_norm"]), total_norm=float(fx[f"total{k}"]))
        assert total.dtype == torch.float32 and total.dim() == 0 and float(total) == float(fx[f"total{k}"])
        assert same_bits(_cat(grads), fx[f"gc{k}"])
        assert all(p.grad is g for p, g in zip(params, grads))
        # unpinned: its own fp64 total, the model's coefficient at it; utils.clip_grad_norm_ on
        # CPU tensors is this loop
        _set_grads(params, inputs[f"g{k}"], lens)
        total = utils.clip_grad_norm_(iter(params), float(inputs["max_norm"]))
        assert GO.ulp_distance(float(total), GO.total(_split(inputs[f"g{k}"], lens))) <= 1
        want = GO.clip(inputs[f"g{k}"], GO.coef(np.float32(float(total)), float(inputs["max_norm"])))
        assert same_bits(_cat([p.grad for p in params]), want)


def test_cpu_clip_grad_norm_skips_parameters_without_gradient_and_other_norms():
    from chocosgd_amd import utils
    a, b = torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2))
    a.grad = torch.tensor([3.0, 4.0, 0.0])
    assert float(utils.clip_grad_norm_([a, b], 1.0)) == 5.0 and b.grad is None
    assert same_bits(a.grad.numpy(), GO.clip(np.array([3, 4, 0], np.float32), GO.coef(5.0, 1.0)))
    assert float(utils.clip_grad_norm_([b], 1.0)) == 0.0
    a.grad = torch.tensor([3.0, -4.0, 0.0])
    assert float(utils.clip_grad_norm_(a, 10.0, norm_type=float("inf"))) == 4.0
    a.grad = torch.tensor([float("inf"), 1.0, 0.0])
    with pytest.raises(RuntimeError, match="non-finite"):
        utils.clip_grad_norm_([a], 1.0, error_if_nonfinite=True)


@pytest.mark.parametrize("write_clipped", [False, True])
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("name", SETS)
def test_cpu_apply_gradient_matches_the_fixtures(inputs, name, flat, write_clipped):
    from chocosgd_amd import utils
    fx = golden(f"gclip_{name}")
    params, groups, lens = _cpu_model(inputs, _hp(fx))
    state = collections.defaultdict(dict)
    out = torch.zeros(sum(lens)) if flat else None
    for k in range(STEPS):
        _set_grads(params, inputs[f"g{k}"], lens)
        grads = [p.grad for p in params]
        utils.apply_gradient(groups, state, flat_out=out, clip_norm=float(inputs["max_norm"]),
                             write_clipped=write_clipped, total_norm=torch.tensor(fx[f"total{k}"]))
        assert same_bits(_cat(params), fx[f"p{k}"]), f"params after step {k}"
        if _hp(fx)[2] != 0:
            assert same_bits(_cat([state[p]["momentum_buffer"] for p in params]), fx[f"buf{k}"])
        assert same_bits(_cat(grads), fx[f"gc{k}"] if write_clipped else inputs[f"g{k}"])
        assert all(p.grad is g for p, g in zip(params, grads))
        if flat:
            assert same_bits(out.numpy(), fx[f"p{k}"])


def test_cpu_apply_gradient_grad_mode_is_clip_then_apply_gradient(inputs):
    from chocosgd_amd import utils
    hp = (0.1, 5e-4, 0.9, 0.0, True)
    a, ga, lens = _cpu_model(inputs, hp)
    b, gb, _ = _cpu_model(inputs, hp)
    sa, sb = collections.defaultdict(dict), collections.defaultdict(dict)
    for k in range(2):
        _set_grads(a, inputs[f"g{k}"], lens)
        _set_grads(b, inputs[f"g{k}"], lens)
        utils.apply_gradient(ga, sa, apply_grad_to_model=False, clip_norm=0.4)
        utils.clip_grad_norm_loop(b, 0.4)
        utils.apply_gradient(gb, sb, apply_grad_to_model=False)
        assert same_bits(_cat([p.grad for p in a]), _cat([p.grad for p in b]))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_cpu_master_clip_is_the_fp32_trajectory(inputs, dtype):
    """apply_gradient(master=, clip_norm=) on CPU tensors: the master follows the fp32 model on
    the widened gradients with the fp32 coefficient, un-narrowed; write_clipped stores the
    narrowed product."""
    from chocosgd_amd import utils
    hp = (0.1, 1e-4, 0.9, 0.0, False)
    tdt = TORCH_DT[dtype]
    params, groups, lens = _cpu_model(inputs, hp, tdt)
    names = [(i, f"p{i}") for i in range(len(params))]
    master = utils.MasterWeights(groups, names)
    state = collections.defaultdict(dict)
    p, buf = SO.to_grid(inputs["p0"], dtype), None
    for k in range(STEPS):
        g = SO.to_grid(inputs[f"g{k}"], dtype)
        _set_grads(params, g, lens, tdt)
        t = GO.total(_split(g, lens))
        gc = GO.clip(g, GO.coef(t, 0.4), "fp32")
        utils.apply_gradient(groups, state, master=master, clip_norm=0.4, write_clipped=True, total_norm=float(t))
        p, buf, _ = SO.sgd_step(p, gc, buf, *hp, first=k == 0)
        assert same_bits(master.buffer.numpy(), p), f"master after step {k}"
        assert same_bits(_cat(params), SO.to_grid(p, dtype))
        assert same_bits(_cat([q.grad for q in params]), SO.to_grid(gc, dtype))


def test_keyword_errors():
    from chocosgd_amd import utils
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.ones(4)
    groups = [{"params": [p], "lr": 0.1, "weight_decay": 0.0, "momentum": 0.0, "dampening": 0.0, "nesterov": False}]
    state = collections.defaultdict(dict)
    with pytest.raises(RuntimeError, match="clip_norm"):
        utils.apply_gradient(groups, state, write_clipped=True)
    with pytest.raises(RuntimeError, match="clip_norm"):
        utils.apply_gradient(groups, state, total_norm=1.0)
    with pytest.raises(RuntimeError, match="write_clipped"):
        utils.apply_gradient(groups, state, apply_grad_to_model=False, clip_norm=1.0, write_clipped=True)
    with pytest.raises(RuntimeError, match="state"):
        utils.fused_step(None, groups, [(0, "p")], None, None, None, 0.5, 0, clip_norm=1.0)
    assert torch.equal(p.data, torch.ones(4)) and torch.equal(p.grad, torch.ones(4))


# ------------------------------------------------------------------ launch and workspace rules
def test_launch_and_workspace_rules(lib):
    from chocosgd_amd import codec
    for nseg, chunks in [(1, 1), (72, 1), (73, 1), (112, 1), (113, 2), (161, 2)]:
        assert lib.choco_params_gradnorm_launches(nseg, 0) == chunks + 1 == codec.params_gradnorm_launches(nseg)
        assert lib.choco_params_gradnorm_launches(nseg, 1) == 1 == codec.params_gradnorm_launches(nseg, pinned=True)
        # the norm pass is choco_params_sqnorm's: the same chunks, and one launch for the total
        assert lib.choco_params_gradnorm_launches(nseg, 0) == lib.choco_params_sqnorm_launches(nseg)
    for nseg in (0, -3):
        assert lib.choco_params_gradnorm_launches(nseg, 0) == 0 == lib.choco_params_gradnorm_launches(nseg, 1)
        assert lib.choco_params_gradnorm_workspace_size(nseg, 100) == 0
    assert lib.choco_params_gradnorm_workspace_size(4, -1) == 0
    # one fp64 slot per (tile, tensor) pair, one fp64 sum and two words per tensor
    for nseg, n in [(1, 0), (72, 8192), (73, 8193), (112, 29414), (113, 29414), (161, 25_557_032)]:
        need = 8 * (n // 8192 + 1 + nseg) + 8 * nseg + 8 * nseg
        sz = lib.choco_params_gradnorm_workspace_size(nseg, n)
        assert sz % 256 == 0 and need <= sz < need + 256, (nseg, n, sz)


# ------------------------------------------------------------------ argument checks (nothing is launched)
def _arr(ct, vals, k):
    return (ct * max(k, 1))(*vals)


def _gclip(lib, p, g, b, lens, dts, n, lr=None, wd=None, mom=None, damp=None, flags=None, flat=0x10000,
           mode=APPLY | WRITE_PARAMS, coef=0x20004, nseg=None, null=(), msg=None, master=False):
    k = len(p)
    tabs = {"params": _arr(ctypes.c_void_p, p, k), "grads": _arr(ctypes.c_void_p, g, k),
            "bufs": _arr(ctypes.c_void_p, b, k), "lens": _arr(ctypes.c_int64, lens, k),
            "dtypes": _arr(ctypes.c_int32, dts, k), "lr": _arr(ctypes.c_double, lr or [0.1] * k, k),
            "wd": _arr(ctypes.c_double, wd or [0.0] * k, k), "mom": _arr(ctypes.c_double, mom or [0.0] * k, k),
            "damp": _arr(ctypes.c_double, damp or [0.0] * k, k), "flags": _arr(ctypes.c_int32, flags or [0] * k, k)}
    a = [None if nm in null else t for nm, t in tabs.items()]
    fn = lib.choco_params_sgd_master_gclip if master else lib.choco_params_sgd_gclip
    return fn(*a, k if nseg is None else nseg, ctypes.c_void_p(flat), n, mode, ctypes.c_void_p(coef), None)


ONE = dict(p=[0x1000], g=[0x2000], b=[0x3000], lens=[4], dts=[F32], n=4)
TWO = dict(p=[0x1000, 0x1100], g=[0x2000, 0x2100], b=[0x3000, 0x3100], lens=[4, 4], dts=[F32, BF16], n=8)
BAD_GCLIP = {
    **{f"null {t}": dict(ONE, null=(t,), msg="null table")
       for t in ["params", "grads", "bufs", "lens", "dtypes", "lr", "wd", "mom", "damp", "flags"]},
    "nseg zero": dict(ONE, nseg=0, msg="nseg"),
    "sum below n": dict(TWO, n=9, msg="add up"),
    "dtype 3": dict(ONE, dts=[3], msg="dtype"),
    "fp32 grad at 2 mod 4": dict(ONE, g=[0x2002], msg="aligned"),
    "null grad": dict(TWO, g=[0, 0x2100], msg="null grad"),
    "null coef": dict(ONE, coef=0, msg="coef"),
    "coef at 2 mod 4": dict(ONE, coef=0x20002, msg="coef"),
    "write_clipped in grad mode": dict(ONE, mode=GRAD | WRITE_GRADS | WRITE_CLIPPED, msg="WRITE_CLIPPED"),
    "write_clipped with a null grad": dict(TWO, g=[0x2000, 0], mode=APPLY | WRITE_CLIPPED, msg="null grad"),
    "add_flat": dict(ONE, mode=GRAD | WRITE_GRADS | ADD_FLAT, msg="ADD_FLAT"),
    "unknown mode bit": dict(ONE, mode=32 | WRITE_PARAMS, msg="mode"),
    "unknown flag bit": dict(ONE, flags=[8], msg="flag"),
    "grad mode writing params": dict(ONE, mode=GRAD | WRITE_PARAMS, msg="grad mode"),
    "apply mode writing grads": dict(ONE, mode=APPLY | WRITE_GRADS, msg="apply mode"),
    "no-grad tensor in grad mode": dict(TWO, mode=GRAD | WRITE_GRADS, flags=[0, NOGRAD], msg="no-grad"),
    "nothing to write": dict(ONE, flat=0, mode=APPLY, msg="nothing to write"),
    "master: null coef": dict(ONE, master=True, coef=0, msg="coef"),
    "master: coef at 2 mod 4": dict(ONE, master=True, coef=0x20002, msg="coef"),
    "master: grad mode": dict(ONE, master=True, mode=GRAD | WRITE_GRADS, msg="master update"),
    "master: write_clipped in grad mode": dict(ONE, master=True, mode=GRAD | WRITE_CLIPPED, msg="master update"),
    "master: add_flat": dict(ONE, master=True, mode=ADD_FLAT, msg="master update"),
    "master: unknown mode bit": dict(ONE, master=True, mode=32, msg="master update"),
    "master: null master": dict(ONE, master=True, flat=0, msg="master is null"),
    "master: write_clipped with a null grad": dict(TWO, master=True, g=[0, 0x2100], mode=WRITE_CLIPPED, msg="null grad"),
    "master: 16-bit momentum buffer": dict(TWO, master=True, b=[0x3000, 0x3102], mom=[0.9, 0.9], msg="aligned"),
}


@pytest.mark.parametrize("case", sorted(BAD_GCLIP))
def test_sgd_gclip_invalid_arguments_are_rejected(lib, case):
    from chocosgd_amd import _lib
    assert _gclip(lib, **BAD_GCLIP[case]) == ERR_INVALID, case
    err = _lib.last_error()
    assert err != "" and BAD_GCLIP[case]["msg"] in err, (case, err)


def test_existing_entry_points_still_reject_write_clipped(lib):
    k = 1
    a = [_arr(ctypes.c_void_p, [0x1000], k), _arr(ctypes.c_void_p, [0x2000], k), _arr(ctypes.c_void_p, [0x3000], k),
         _arr(ctypes.c_int64, [4], k), _arr(ctypes.c_int32, [F32], k)] + [_arr(ctypes.c_double, [0.0], k)] * 4 + \
        [_arr(ctypes.c_int32, [0], k)]
    assert lib.choco_params_sgd(*a, 1, ctypes.c_void_p(0x10000), 4, WRITE_PARAMS | WRITE_CLIPPED, None) == ERR_INVALID
    assert lib.choco_params_sgd_master(*a, 1, ctypes.c_void_p(0x10000), 4, WRITE_CLIPPED, None) == ERR_INVALID
    assert lib.choco_params_sgd_clip(*a, 1, ctypes.c_void_p(0x10000), 4, WRITE_PARAMS | WRITE_CLIPPED, None, 0.0,
                                     None) == ERR_INVALID


def _gradnorm(lib, g, lens, dts, n, flags=None, max_norm=0.4, cd=F32, total_in=0, out=0x20000, norms=0x21000,
              ws=0x30000, ws_bytes=1 << 20, nseg=None, null=(), msg=None, rc=None):
    k = len(g)
    tabs = {"grads": _arr(ctypes.c_void_p, g, k), "lens": _arr(ctypes.c_int64, lens, k),
            "dtypes": _arr(ctypes.c_int32, dts, k), "flags": _arr(ctypes.c_int32, flags or [0] * k, k)}
    a = [None if nm in null else t for nm, t in tabs.items()]
    return lib.choco_params_gradnorm(*a, k if nseg is None else nseg, n, max_norm, cd, ctypes.c_void_p(total_in),
                                     ctypes.c_void_p(out), ctypes.c_void_p(norms), ctypes.c_void_p(ws), ws_bytes, None)


N1 = dict(g=[0x2000], lens=[4], dts=[F32], n=4)
N2 = dict(g=[0x2000, 0x2100], lens=[4, 4], dts=[F32, F16], n=8)
BAD_GRADNORM = {
    **{f"null {t}": dict(N1, null=(t,), msg="null table") for t in ["grads", "lens", "dtypes", "flags"]},
    "nseg zero": dict(N1, nseg=0, msg="nseg"),
    "nseg negative": dict(N1, nseg=-1, msg="nseg"),
    "negative length": dict(N2, lens=[-4, 8], n=4, msg="negative length"),
    "sum below n": dict(N2, n=9, msg="add up"),
    "sum above n": dict(N2, n=7, msg="add up"),
    "n = 2^31": dict(N1, lens=[2 ** 31], n=2 ** 31, msg="2^31"),
    "dtype 3": dict(N1, dts=[3], msg="dtype"),
    "fp32 grad at 2 mod 4": dict(N1, g=[0x2002], msg="aligned"),
    "fp16 grad at odd byte": dict(N2, g=[0x2000, 0x2101], msg="aligned"),
    "null grad": dict(N2, g=[0, 0x2100], msg="null grad"),
    "unknown flag bit": dict(N1, flags=[8], msg="flag"),
    "max_norm nan": dict(N1, max_norm=float("nan"), msg="max_norm"),
    "max_norm negative": dict(N1, max_norm=-0.5, msg="max_norm"),
    "max_norm inf": dict(N1, max_norm=float("inf"), msg="max_norm"),
    "max_norm past fp32": dict(N1, max_norm=1e39, msg="max_norm"),
    "coef_dtype 3": dict(N1, cd=3, msg="coef_dtype"),
    "coef_dtype negative": dict(N1, cd=-1, msg="coef_dtype"),
    "null out": dict(N1, out=0, msg="out"),
    "out at 2 mod 4": dict(N1, out=0x20002, msg="out"),
    "norms at 2 mod 4": dict(N1, norms=0x21002, msg="norms"),
    "total_in at 2 mod 4": dict(N1, total_in=0x22002, norms=0, msg="total_in"),
    "norms with a pinned total": dict(N1, total_in=0x22000, msg="pinned"),
    "pinned: max_norm nan": dict(N1, total_in=0x22000, norms=0, max_norm=float("nan"), msg="max_norm"),
    "pinned: null out": dict(N1, total_in=0x22000, norms=0, out=0, msg="out"),
    "null workspace": dict(N1, ws=0, msg="workspace"),
    "workspace at 4 mod 8": dict(N1, ws=0x30004, msg="workspace"),
    "short workspace": dict(N1, ws_bytes=16, msg="workspace too small", rc=ERR_WORKSPACE),
}


@pytest.mark.parametrize("case", sorted(BAD_GRADNORM))
def test_gradnorm_invalid_arguments_are_rejected(lib, case):
    from chocosgd_amd import _lib
    assert _gradnorm(lib, **BAD_GRADNORM[case]) == (BAD_GRADNORM[case].get("rc") or ERR_INVALID), case
    err = _lib.last_error()
    assert err != "" and BAD_GRADNORM[case]["msg"] in err, (case, err)


def test_plan_keyword_errors_need_no_device():
    """ParamSgdPlan.run refuses gclip together with DGC's keywords before it touches a tensor."""
    from chocosgd_amd import codec
    plan = object.__new__(codec.ParamSgdPlan)
    plan.n, plan.nseg, plan.device = 4, 1, torch.device("cpu")
    marker = object()
    for kw in (dict(norms=marker), dict(clip_threshold=1.0, norms=marker), dict(add_flat=True)):
        with pytest.raises(RuntimeError, match="does not combine"):
            plan.run(None, gclip=marker, **kw)
    with pytest.raises(RuntimeError, match="write_clipped"):
        plan.run(None, write_clipped=True)
    with pytest.raises(RuntimeError, match="apply mode"):
        plan.run(None, grad_mode=True, gclip=marker, write_clipped=True)
