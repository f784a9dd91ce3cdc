"""DGC's optimizer half, host side (no GPU): the numpy model (_dgc_oracle) and
dgc.apply_gradient's per-tensor loop against the reference's fixtures (tests/golden/dgc_sgd_*.npz,
gen_golden_dgc_sgd.py), bit for bit with the fixture's norms pinned; the launch-count rules; the
argument checks of choco_params_sqnorm, choco_params_sgd_clip and choco_params_mask, made before
any HIP call."""
import collections
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import golden, same_bits
import _dgc_oracle as DO

ERR_INVALID, ERR_WORKSPACE = -1, -3
F32, BF16, F16 = 0, 1, 2
NESTEROV, FIRST, NOGRAD = 1, 2, 4
APPLY, GRAD, WRITE_PARAMS, WRITE_GRADS, ADD_FLAT = 0, 1, 2, 4, 8
SETS = ["clip", "wd", "mom", "nesterov", "damp"]
STEPS = 3


@pytest.fixture(scope="module")
def lib():
    from chocosgd_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def inputs():
    return golden("dgc_sgd_inputs")


def _hp(fx):
    lr, wd, mom, damp, nest = fx["hp"].tolist()
    return lr, wd, mom, damp, bool(nest)


def test_fixture_threshold_is_the_reference_expression(inputs):
    val, n_nodes = float(inputs["clip_grad_val"]), int(inputs["n_nodes"])
    from chocosgd_amd import dgc
    assert dgc._clip_threshold(True, val, n_nodes) == float(inputs["thr"]) == val * (1.0 / math.sqrt(n_nodes))
    assert dgc._clip_threshold(False, val, n_nodes) is None and dgc._clip_threshold(True, None, n_nodes) is None


def test_fixture_pins_the_comparison(inputs):
    """The last tensor's norm equals (float)thr exactly and it IS clipped, with changed bits; the
    double comparison would leave it alone when (float)thr < thr."""
    thr = float(inputs["thr"])
    fx = golden("dgc_sgd_clip")
    for k in range(STEPS):
        assert fx[f"norm{k}"][-1] == np.float32(thr)
        assert fx[f"d{k}"][-1] != inputs[f"g{k}"][-1]
        assert DO.clip_coef(fx[f"norm{k}"][-1], thr) != np.float32(1)


@pytest.mark.parametrize("name", SETS)
def test_oracle_matches_the_reference_fixtures(inputs, name):
    fx = golden(f"dgc_sgd_{name}")
    hp, lens, thr = _hp(fx), inputs["lens"].tolist(), float(inputs["thr"])
    buf = None
    for k in range(STEPS):
        _, buf, d = DO.step_layout(inputs["p0"], inputs[f"g{k}"], buf, lens, hp, k == 0, fx[f"norm{k}"], thr)
        assert same_bits(d, fx[f"d{k}"]), f"d_p after step {k}"
        if hp[2] != 0:
            assert same_bits(buf, fx[f"buf{k}"]), f"buf after step {k}"


@pytest.mark.parametrize("name", SETS)
def test_oracle_norms_are_next_to_the_reference_norms(inputs, name):
    """The model's fp64 norm against torch's fp32-accumulated one: equal or adjacent fp32 values
    (a sanity check of the model's d; the kernels are held to the fp64 value)."""
    fx = golden(f"dgc_sgd_{name}")
    hp, lens = _hp(fx), inputs["lens"].tolist()
    for k in range(STEPS):
        mine = DO.norms_layout(inputs["p0"], inputs[f"g{k}"], lens, hp[1])
        ref = fx[f"norm{k}"]
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(mine), np.isnan(ref)) and np.array_equal(np.isinf(mine), np.isinf(ref))
        assert np.all(np.abs(mine[fin].view(np.int32) - ref[fin].view(np.int32)) <= 2), (mine, ref)


def _cpu_model(inputs, hp):
    lr, wd, mom, damp, nest = hp
    lens = inputs["lens"].tolist()
    params, o = [], 0
    for m in lens:
        params.append(torch.nn.Parameter(torch.from_numpy(inputs["p0"][o:o + m].copy())))
        o += m
    groups = [{"params": [p], "lr": lr, "weight_decay": wd, "momentum": mom, "dampening": damp, "nesterov": nest}
              for p in params]
    return params, groups, lens


def _set_grads(params, flat, lens):
    o = 0
    for p, m in zip(params, lens):
        p.grad = torch.from_numpy(flat[o:o + m].copy())
        o += m


def _cat(tensors):
    return np.concatenate([t.detach().float().numpy().reshape(-1) for t in tensors])


@pytest.mark.parametrize("flat_mode", ["none", "flat", "add_flat"])
@pytest.mark.parametrize("name", SETS)
def test_cpu_apply_gradient_matches_the_reference_fixtures(inputs, name, flat_mode):
    from chocosgd_amd import dgc
    fx = golden(f"dgc_sgd_{name}")
    hp = _hp(fx)
    params, groups, lens = _cpu_model(inputs, hp)
    state = collections.defaultdict(dict)
    val, n_nodes = float(inputs["clip_grad_val"]), int(inputs["n_nodes"])
    mem0 = np.linspace(-2, 2, sum(lens)).astype(np.float32)
    flat = None if flat_mode == "none" else torch.from_numpy(mem0.copy())
    for k in range(STEPS):
        _set_grads(params, inputs[f"g{k}"], lens)
        grads = [p.grad for p in params]
        before = None if flat is None else flat.numpy().copy()
        used = dgc.apply_gradient(groups, state, clip_grad=True, clip_grad_val=val, n_nodes=n_nodes, flat_out=flat,
                                  add_flat=flat_mode == "add_flat", norms=torch.from_numpy(fx[f"norm{k}"]))
        assert same_bits(used.numpy(), fx[f"norm{k}"])
        assert same_bits(_cat(grads), fx[f"d{k}"]), f"d_p after step {k}"
        assert same_bits(_cat(params), inputs["p0"]), "the parameters are not touched"
        assert all(p.grad is g for p, g in zip(params, grads)), "p.grad must not be rebound"
        if hp[2] != 0:
            assert same_bits(_cat([state[p]["momentum_buffer"] for p in params]), fx[f"buf{k}"]), f"buf, step {k}"
        if flat_mode == "flat":
            assert same_bits(flat.numpy(), fx[f"d{k}"])
        elif flat_mode == "add_flat":
            with np.errstate(all="ignore"):
                assert same_bits(flat.numpy(), before + fx[f"d{k}"])


@pytest.mark.parametrize("name", ["clip", "nesterov"])
def test_cpu_apply_gradient_unpinned_matches_the_model_at_its_own_norms(inputs, name):
    from chocosgd_amd import dgc
    fx = golden(f"dgc_sgd_{name}")
    hp = _hp(fx)
    params, groups, lens = _cpu_model(inputs, hp)
    state = collections.defaultdict(dict)
    val, n_nodes, thr = float(inputs["clip_grad_val"]), int(inputs["n_nodes"]), float(inputs["thr"])
    buf = None
    for k in range(STEPS):
        _set_grads(params, inputs[f"g{k}"], lens)
        used = dgc.apply_gradient(groups, state, clip_grad=True, clip_grad_val=val, n_nodes=n_nodes)
        assert used.dtype == torch.float32 and used.numel() == len(lens)
        _, buf, d = DO.step_layout(inputs["p0"], inputs[f"g{k}"], buf, lens, hp, k == 0, used.numpy(), thr)
        assert same_bits(_cat([p.grad for p in params]), d), f"d_p after step {k}"
        if hp[2] != 0:
            assert same_bits(_cat([state[p]["momentum_buffer"] for p in params]), buf)


def test_cpu_apply_gradient_without_clipping_is_apply_gradient(inputs):
    """clip_grad False (or no clip_grad_val): utils.apply_gradient's grad mode, and no norms."""
    from chocosgd_amd import dgc, utils
    hp = (0.1, 5e-4, 0.9, 0.0, True)
    a, ga, lens = _cpu_model(inputs, hp)
    b, gb, _ = _cpu_model(inputs, hp)
    sa, sb = collections.defaultdict(dict), collections.defaultdict(dict)
    for k in range(2):
        _set_grads(a, inputs[f"g{k}"], lens)
        _set_grads(b, inputs[f"g{k}"], lens)
        assert dgc.apply_gradient(ga, sa, clip_grad=k == 0, clip_grad_val=None) is None
        utils.apply_gradient(gb, sb, apply_grad_to_model=False)
        assert same_bits(_cat([p.grad for p in a]), _cat([p.grad for p in b]))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["clip", "nesterov"])
def test_cpu_loop_16_bit_clips_with_the_kernel_coefficient(inputs, name, dtype):
    """The per-tensor loop on 16-bit tensors keeps the clip coefficient in fp32 and narrows the
    product once, as the batched kernel does: with the model's norms fed in, d_p after the clip
    line matches the model bit for bit (weight decay and momentum off: only that line runs)."""
    from chocosgd_amd import dgc
    import _sgd_oracle as SO
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    wd = _hp(golden(f"dgc_sgd_{name}"))[1]
    hp = (0.1, 0.0, 0.0, 0.0, False)
    params, groups, lens = _cpu_model(inputs, hp)
    for p in params:
        p.data = p.data.to(tdt)
    val, n_nodes, thr = float(inputs["clip_grad_val"]), int(inputs["n_nodes"]), float(inputs["thr"])
    p0 = SO.to_grid(inputs["p0"], dtype)
    for k in range(STEPS):
        # the decayed gradient of the set as this step's gradient, on the dtype's grid
        g = DO.decayed(p0, SO.to_grid(inputs[f"g{k}"], dtype), wd, dtype)
        o = 0
        for p, m in zip(params, lens):
            p.grad = torch.from_numpy(g[o:o + m].copy()).to(tdt)
            o += m
        norms = DO.norms_layout(p0, g, lens, 0.0, dtype)
        coefs = [DO.clip_coef(v, thr) for v in norms]
        assert any(c != 1 and SO.to_grid(np.array([c], np.float32), dtype)[0] != c for c in coefs), \
            "no coefficient off the 16-bit grid: the case shows nothing"
        dgc.apply_gradient_loop(groups, collections.defaultdict(dict), clip_grad=True, clip_grad_val=val,
                                n_nodes=n_nodes, norms=torch.from_numpy(norms))
        _, _, d = DO.step_layout(p0, g, None, lens, hp, True, norms, thr, dtype)
        assert same_bits(_cat([p.grad for p in params]), d), f"d_p after step {k}"


def test_fused_step_refuses_the_strict_mask_before_it_steps():
    from chocosgd_amd import dgc
    from chocosgd_amd.tensor_buffer import TensorBuffer
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.full((4,), 0.5)
    groups = [{"params": [p], "lr": 0.1, "weight_decay": 1e-2, "momentum": 0.9, "dampening": 0.0, "nesterov": False,
               "name": "p0"}]
    state = collections.defaultdict(dict)
    mem = TensorBuffer([torch.zeros(4)])
    c = dgc.DGCCodec(None, "compress_top_k", "gpu", 3, strict_reference=True)
    with pytest.raises(RuntimeError, match="strict_reference"):
        dgc.fused_step(c, groups, [(0, "p0")], state, mem, 0.5, clip_grad=True, clip_grad_val=1.0,
                       mask_momentum=True)
    assert torch.equal(p.grad, torch.full((4,), 0.5)) and torch.equal(mem.buffer, torch.zeros(4))
    assert "momentum_buffer" not in state[p] and torch.equal(p.data, torch.ones(4))


def test_negative_momentum_is_refused():
    from chocosgd_amd import dgc
    p = torch.nn.Parameter(torch.ones(3))
    p.grad = torch.ones(3)
    groups = [{"params": [p], "lr": 0.1, "weight_decay": 0.0, "momentum": -0.5, "dampening": 0.0, "nesterov": False}]
    for fn in (dgc.apply_gradient, dgc.apply_gradient_loop):
        with pytest.raises(RuntimeError, match="momentum"):
            fn(groups, collections.defaultdict(dict))


def test_strict_reference_refuses_momentum_buffers():
    from chocosgd_amd.dgc import DGCCodec
    from chocosgd_amd.tensor_buffer import TensorBuffer
    c = DGCCodec(None, "compress_top_k", "gpu", 3, strict_reference=True)
    g = [torch.ones(4)]
    with pytest.raises(RuntimeError, match="strict_reference"):
        c.compress(g, TensorBuffer([torch.zeros(4)]), 0.5, momentum_buffers=[torch.zeros(4)])
    q = DGCCodec(None, "quantize_qsgd", "gpu", 3, quantize_level=4, strict_reference=False)
    with pytest.raises(RuntimeError, match="quantize"):
        q.compress(g, TensorBuffer([torch.zeros(4)]), 0.5, grads_in_memory=True)


def test_oracle_mask_model():
    lens, ks = [4, 0, 3], [2, 0, 1]
    bufs = [np.array([1, -3, np.inf, 2], np.float32), None, np.array([np.nan, -5, 7], np.float32)]
    mem = np.arange(7, dtype=np.float32) + 1
    vals = np.array([2, np.inf, 6], np.float32)
    DO.mask(bufs, ["fp32"] * 3, lens, vals, np.array([1, 2, 5]), ks, mem)
    assert same_bits(bufs[0], np.array([1, -0.0, np.nan, 2], np.float32))
    assert same_bits(bufs[2], np.array([np.nan, -0.0, 7], np.float32))
    assert same_bits(mem, np.array([1, 0, np.nan, 4, 5, 0, 7], np.float32))
    # an index outside its tensor's range is skipped
    b2 = [np.ones(4, np.float32), None, np.ones(3, np.float32)]
    DO.mask(b2, ["fp32"] * 3, lens, vals, np.array([1, 5, 3]), ks, None)
    assert b2[0].tolist() == [1, 0, 1, 1] and b2[2].tolist() == [1, 1, 1]


def test_launch_rules(lib):
    from chocosgd_amd import codec
    for nseg in [1, 111, 112, 113, 300, 3000]:
        assert lib.choco_params_sqnorm_launches(nseg) == -(-nseg // 112) + 1 == codec.params_sqnorm_launches(nseg)
        assert lib.choco_params_mask_launches(nseg) == -(-nseg // 128) == codec.params_mask_launches(nseg)
    assert lib.choco_params_sqnorm_launches(161) == 3  # ResNet-50: two chunks and the finish
    for f in (lib.choco_params_sqnorm_launches, lib.choco_params_mask_launches):
        assert f(0) == 0 and f(-4) == 0
    # one fp64 slot per (tile, tensor) pair and two words per tensor
    for nseg, n in [(1, 0), (10, 29414), (161, 25_557_032), (3000, 300_000)]:
        sz = lib.choco_params_sqnorm_workspace_size(nseg, n)
        assert sz % 256 == 0 and sz >= 8 * (n // 8192 + 1 + nseg) + 8 * nseg
        assert sz < 8 * (n // 8192 + 1 + nseg) + 8 * nseg + 256
    assert lib.choco_params_sqnorm_workspace_size(0, 10) == 0


# ------------------------------------------------------------------ argument checks (nothing is launched)
def _arr(ct, vals, k):
    return (ct * max(k, 1))(*vals)


def _sgd_clip(lib, p, g, b, lens, dts, n, lr=None, wd=None, mom=None, damp=None, flags=None, flat=0x10000,
              mode=GRAD | WRITE_GRADS, norms=0x20000, thr=1.0, nseg=None, null=(), msg=None, entry="clip"):
    k = len(p)
    tabs = {"params": _arr(ctypes.c_void_p, p, k), "grads": _arr(ctypes.c_void_p, g, k),
            "bufs": _arr(ctypes.c_void_p, b, k), "lens": _arr(ctypes.c_int64, lens, k),
            "dtypes": _arr(ctypes.c_int32, dts, k), "lr": _arr(ctypes.c_double, lr or [0.1] * k, k),
            "wd": _arr(ctypes.c_double, wd or [0.0] * k, k), "mom": _arr(ctypes.c_double, mom or [0.0] * k, k),
            "damp": _arr(ctypes.c_double, damp or [0.0] * k, k), "flags": _arr(ctypes.c_int32, flags or [0] * k, k)}
    a = [None if nm in null else t for nm, t in tabs.items()]
    ns = k if nseg is None else nseg
    if entry == "plain":
        return lib.choco_params_sgd(*a, ns, ctypes.c_void_p(flat), n, mode, None)
    return lib.choco_params_sgd_clip(*a, ns, ctypes.c_void_p(flat), n, mode, ctypes.c_void_p(norms), thr, None)


ONE = dict(p=[0x1000], g=[0x2000], b=[0x3000], lens=[4], dts=[F32], n=4)
TWO = dict(p=[0x1000, 0x1100], g=[0x2000, 0x2100], b=[0x3000, 0x3100], lens=[4, 4], dts=[F32, BF16], n=8)
BAD_CLIP = {
    **{f"null {t}": dict(ONE, null=(t,), msg="null table")
       for t in ["params", "grads", "bufs", "lens", "dtypes", "lr", "wd", "mom", "damp", "flags"]},
    "nseg zero": dict(ONE, nseg=0, msg="nseg"),
    "sum below n": dict(TWO, n=9, msg="add up"),
    "dtype 3": dict(ONE, dts=[3], msg="dtype"),
    "fp32 grad at 2 mod 4": dict(ONE, g=[0x2002], msg="aligned"),
    "null grad": dict(TWO, g=[0, 0x2100], msg="null grad"),
    "threshold zero": dict(ONE, thr=0.0, msg="threshold"),
    "threshold negative": dict(ONE, thr=-1.0, msg="threshold"),
    "threshold inf": dict(ONE, thr=float("inf"), msg="threshold"),
    "threshold nan": dict(ONE, thr=float("nan"), msg="threshold"),
    "threshold past fp32": dict(ONE, thr=1e39, msg="threshold"),
    "threshold below fp32 (0 as a float)": dict(ONE, thr=1e-50, msg="threshold"),
    "norms at 2 mod 4": dict(ONE, norms=0x20002, msg="norms"),
    "add_flat in apply mode": dict(ONE, mode=APPLY | WRITE_PARAMS | ADD_FLAT, msg="ADD_FLAT"),
    "add_flat without flat": dict(ONE, flat=0, mode=GRAD | WRITE_GRADS | ADD_FLAT, msg="ADD_FLAT"),
    "unknown mode bit": dict(ONE, mode=16 | GRAD | WRITE_GRADS, msg="mode"),
    "unknown flag bit": dict(ONE, flags=[8], msg="flag"),
    "grad mode writing params": dict(ONE, mode=GRAD | WRITE_PARAMS, msg="grad mode"),
    "no-grad tensor in grad mode": dict(TWO, flags=[0, NOGRAD], msg="no-grad"),
    "nothing to write": dict(ONE, flat=0, mode=GRAD, msg="nothing to write"),
    "plain entry point, add_flat": dict(ONE, mode=GRAD | WRITE_GRADS | ADD_FLAT, entry="plain", msg="mode"),
    "plain entry point, flag bit 8": dict(ONE, flags=[8], entry="plain", msg="flag"),
}


@pytest.mark.parametrize("case", sorted(BAD_CLIP))
def test_sgd_clip_invalid_arguments_are_rejected(lib, case):
    from chocosgd_amd import _lib
    assert _sgd_clip(lib, **BAD_CLIP[case]) == ERR_INVALID, case
    err = _lib.last_error()
    assert err != "" and BAD_CLIP[case]["msg"] in err, (case, err)


def _sqnorm(lib, p, g, lens, dts, n, wd=None, flags=None, norms=0x20000, ws=0x30000, ws_bytes=1 << 20, nseg=None,
            null=(), msg=None, rc=None):
    k = len(p)
    tabs = {"params": _arr(ctypes.c_void_p, p, k), "grads": _arr(ctypes.c_void_p, g, k),
            "lens": _arr(ctypes.c_int64, lens, k), "dtypes": _arr(ctypes.c_int32, dts, k),
            "wd": _arr(ctypes.c_double, wd or [0.0] * k, k), "flags": _arr(ctypes.c_int32, flags or [0] * k, k)}
    a = [None if nm in null else t for nm, t in tabs.items()]
    return lib.choco_params_sqnorm(*a, k if nseg is None else nseg, n, ctypes.c_void_p(norms), ctypes.c_void_p(ws),
                                   ws_bytes, None)


N1 = dict(p=[0x1000], g=[0x2000], lens=[4], dts=[F32], n=4)
N2 = dict(p=[0x1000, 0x1100], g=[0x2000, 0x2100], lens=[4, 4], dts=[F32, F16], n=8)
BAD_NORM = {
    **{f"null {t}": dict(N1, null=(t,), msg="null table") for t in ["params", "grads", "lens", "dtypes", "wd", "flags"]},
    "nseg zero": dict(N1, nseg=0, msg="nseg"),
    "nseg negative": dict(N1, nseg=-1, msg="nseg"),
    "negative length": dict(N2, lens=[-4, 8], n=4, msg="negative length"),
    "sum below n": dict(N2, n=9, msg="add up"),
    "sum above n": dict(N2, n=7, msg="add up"),
    "n = 2^31": dict(N1, lens=[2 ** 31], n=2 ** 31, msg="2^31"),
    "dtype 3": dict(N1, dts=[3], msg="dtype"),
    "fp32 grad at 2 mod 4": dict(N1, g=[0x2002], msg="aligned"),
    "fp16 param at odd byte": dict(N2, p=[0x1000, 0x1101], msg="aligned"),
    "null grad": dict(N2, g=[0, 0x2100], msg="null grad"),
    "null param with weight decay": dict(N2, p=[0x1000, 0], wd=[0.0, 1e-4], msg="null param"),
    "unknown flag bit": dict(N1, flags=[8], msg="flag"),
    "null norms": dict(N1, norms=0, msg="norms"),
    "norms at 2 mod 4": dict(N1, norms=0x20002, msg="norms"),
    "null workspace": dict(N1, ws=0, msg="workspace"),
    "workspace at 4 mod 8": dict(N1, ws=0x30004, msg="workspace"),
    "short workspace": dict(N1, ws_bytes=16, msg="workspace too small", rc=ERR_WORKSPACE),
}


@pytest.mark.parametrize("case", sorted(BAD_NORM))
def test_sqnorm_invalid_arguments_are_rejected(lib, case):
    from chocosgd_amd import _lib
    assert _sqnorm(lib, **BAD_NORM[case]) == (BAD_NORM[case].get("rc") or ERR_INVALID), case
    err = _lib.last_error()
    assert err != "" and BAD_NORM[case]["msg"] in err, (case, err)


def _mask(lib, b, lens, dts, ks, n, k=None, values=0x40000, indices=0x50000, memory=0x60000, nseg=None, null=(),
          msg=None):
    m = len(b)
    tabs = {"bufs": _arr(ctypes.c_void_p, b, m), "lens": _arr(ctypes.c_int64, lens, m),
            "dtypes": _arr(ctypes.c_int32, dts, m), "ks": _arr(ctypes.c_int64, ks, m)}
    a = [None if nm in null else t for nm, t in tabs.items()]
    return lib.choco_params_mask(*a, m if nseg is None else nseg, ctypes.c_void_p(values), ctypes.c_void_p(indices),
                                 sum(ks) if k is None else k, ctypes.c_void_p(memory), n, None)


M1 = dict(b=[0x1000], lens=[4], dts=[F32], ks=[2], n=4)
M2 = dict(b=[0x1000, 0x1100], lens=[4, 4], dts=[F32, BF16], ks=[1, 2], n=8)
BAD_MASK = {
    **{f"null {t}": dict(M1, null=(t,), msg="null table") for t in ["bufs", "lens", "dtypes", "ks"]},
    "nseg zero": dict(M1, nseg=0, msg="nseg"),
    "negative length": dict(M2, lens=[-4, 8], ks=[0, 2], n=4, msg="negative length"),
    "sum below n": dict(M2, n=9, msg="add up"),
    "sum above n": dict(M2, n=7, msg="add up"),
    "n = 2^31": dict(M1, lens=[2 ** 31], n=2 ** 31, msg="2^31"),
    "dtype 3": dict(M1, dts=[3], msg="dtype"),
    "negative k_per_seg": dict(M2, ks=[-1, 2], k=1, msg="k_per_seg"),
    "k_per_seg above the length": dict(M2, ks=[5, 0], msg="k_per_seg"),
    "k_per_seg does not add up to k": dict(M2, k=4, msg="k_per_seg adds up"),
    "negative k": dict(M1, k=-1, msg="k must"),
    "null values": dict(M1, values=0, msg="null values"),
    "null indices": dict(M1, indices=0, msg="null values"),
    "indices at 2 mod 4": dict(M1, indices=0x50002, msg="4-byte"),
    "memory at 2 mod 4": dict(M1, memory=0x60002, msg="4-byte"),
    "fp32 buf at 2 mod 4": dict(M1, b=[0x1002], msg="aligned"),
    "bf16 buf at odd byte": dict(M2, b=[0x1000, 0x1101], msg="aligned"),
    "nothing to write": dict(M2, b=[0, 0], memory=0, msg="nothing to write"),
}


@pytest.mark.parametrize("case", sorted(BAD_MASK))
def test_mask_invalid_arguments_are_rejected(lib, case):
    from chocosgd_amd import _lib
    assert _mask(lib, **BAD_MASK[case]) == ERR_INVALID, case
    err = _lib.last_error()
    assert err != "" and BAD_MASK[case]["msg"] in err, (case, err)
