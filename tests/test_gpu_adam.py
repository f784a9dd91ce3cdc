"""The batched Adam / AdamW update on the device: codec.params_adam and
codec.params_adam_master (csrc/adam.hip) and the layers above them (utils.apply_adam,
utils.fused_step(state=, update="adam")).

Everything is compared bit for bit against the numpy restatement of the documented per-element
lines (tests/_adam_oracle.py), whole guarded storages at a time (test_gpu_param_sgd.py's), so
that every byte a launch does not own is checked together with the ones it does."""
import collections

import numpy as np
import pytest
import torch

from conftest import golden_json, same_bits
import _adam_oracle as AO
import _sgd_oracle as SO
import test_gpu_param_sgd as PS
from test_gpu_param_sgd import DTYPES, NAMES, SENTINEL, Guarded, _dtypes, _values, host

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 54  # tensors per launch (adam.hip kAdamCap)
MODES = ["fp32", "bf16", "fp16", "mixed"]
BASE = [1, 2, 3, 7, 8, 9, 31, 33, 4097, 16, 8200, 20]
SIDES = ["plain", "master"]
COEF = float(np.float32(0.37))


def _counts():
    from chocosgd_amd import codec
    return (codec.launch_count("param_adam_kernel"), codec.launch_count("param_adam_master_kernel"),
            codec.launch_count("param_pack_kernel"))


def _varied_hp(i):
    """lr, beta1, beta2, eps, wd, step, decoupled differing inside one launch: both branches of
    the lerp, no weight decay on one tensor in four, AdamW's and Adam's decay alternating."""
    return 1e-3 * (1 + i % 5), 0.4 if i % 3 == 1 else 0.9, 0.999, 1e-8, 0.0 if i % 4 == 2 else 0.01, 1 + i % 7, i % 2 == 0


def _abs(guarded):
    """exp_avg_sq is a sum of squares: the storages' magnitudes (the guards become +7)."""
    for s in guarded.stores:
        s.copy_(s.abs())
    guarded.before = [s.clone() for s in guarded.stores]
    return guarded


def run_case(lens, mode, side="plain", lead=(0, 0, 0, 0), gap=8, own=False, flat_shift=4, nograd=(), hp=_varied_hp,
             first=lambda i: i % 2 == 0, write=True, coef=None, write_clipped=False, seed=1000, m_range=(-4, 0),
             v_range=(-7, 0)):
    """One codec.params_adam / params_adam_master call on guarded storages against the oracle;
    returns the launches."""
    from chocosgd_amd import codec
    master = side == "master"
    k, n = len(lens), sum(lens)
    dts = _dtypes(mode, k)
    mdts = [torch.float32] * k if master else dts  # a master update's moments are fp32
    P = Guarded(lens, dts, seed, -3, 1, lead[0], gap, own)
    G = Guarded(lens, dts, seed + 5000, -4, 0, lead[1], gap, own)
    M = Guarded(lens, mdts, seed + 9000, *m_range, lead[2], gap, own)
    V = _abs(Guarded(lens, mdts, seed + 13000, *v_range, lead[3], gap, own))
    hps = [hp(i) for i in range(k)]
    firsts = [bool(first(i)) for i in range(k)]
    big = flat = None
    if flat_shift is not None:
        big = torch.full((n + 2 * flat_shift + 8,), SENTINEL, device=DEV)
        flat = big[flat_shift:flat_shift + n]
        if master and n:
            flat.copy_(torch.from_numpy(_values(n, seed + 17000, -3, 1)).to(DEV))
    before_flat = None if flat is None else host(flat)
    gclip = None if coef is None else torch.tensor([1.0, coef], device=DEV)
    new_p, new_g, new_m, new_v, new_flat = [], [], [], [], []
    o = 0
    for i in range(k):
        pw, gw, mw, vw = host(P.views[i]), host(G.views[i]), host(M.views[i]), host(V.views[i])
        sl = slice(o, o + lens[i])
        o += lens[i]
        if i in nograd:
            new_p.append(None), new_g.append(None), new_m.append(None), new_v.append(None)
            new_flat.append(before_flat[sl] if master else pw)
            continue
        lr, b1, b2, eps, wd, step, dec = hps[i]
        if master:
            x_new, m_new, v_new, p_new, g_c = AO.adam_master_step(before_flat[sl], gw, mw, vw, lr, b1, b2, eps, wd, step,
                                                                  dec, firsts[i], coef, dtype=NAMES[dts[i]])
            new_flat.append(x_new)
        else:
            p_new, m_new, v_new, g_c = AO.adam_step(pw, gw, mw, vw, lr, b1, b2, eps, wd, step, dec, firsts[i], coef,
                                                    dtype=NAMES[dts[i]])
            new_flat.append(p_new)
        new_p.append(p_new if write else None)
        new_g.append(g_c if write_clipped else None)
        new_m.append(m_new)
        new_v.append(v_new)
    c0 = _counts()
    args = (P.views, [None if i in nograd else g for i, g in enumerate(G.views)], M.views, V.views,
            [h[0] for h in hps], [(h[1], h[2]) for h in hps], [h[3] for h in hps], [h[4] for h in hps],
            [h[5] for h in hps], [h[6] for h in hps], firsts)
    if master:
        codec.params_adam_master(*args, master=flat, write=write, gclip=gclip, write_clipped=write_clipped)
    else:
        codec.params_adam(*args, flat=flat, write=write, gclip=gclip, write_clipped=write_clipped)
    c1 = _counts()
    P.check(new_p, "params (or their guards)")
    G.check(new_g, "grads (or their guards)")
    M.check(new_m, "exp_avg (or its guards)")
    V.check(new_v, "exp_avg_sq (or its guards)")
    if flat is not None:
        want = torch.full_like(big, SENTINEL)
        if n:
            want[flat_shift:flat_shift + n] = torch.from_numpy(np.concatenate(new_flat).astype(np.float32)).to(DEV)
        assert same_bits(host(big), host(want)), "flat / master (or its guards)"
    launches = [b - a for a, b in zip(c0, c1)]
    assert launches == ([0, codec.params_adam_launches(k), 0] if master else [codec.params_adam_launches(k), 0, 0])
    return launches[1 if master else 0]


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("mode", MODES)
def test_cut_groups_and_tile_crossings(mode, side):
    """One storage per dtype, every tensor eight elements further in than its flat offset: the
    16-byte path with cut groups at both ends, FIRST on every other tensor, then on none and
    on all."""
    run_case(BASE, mode, side)
    run_case(BASE, mode, side, first=lambda i: False, coef=COEF)
    run_case(BASE, mode, side, first=lambda i: True, coef=COEF, write_clipped=True)


@pytest.mark.parametrize("which", range(4))
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("mode", MODES)
def test_views_at_every_offset_of_a_group(mode, side, which):
    """p, g, m or v alone 1 to 7 elements into its allocation, the other three aligned (each
    tensor its own allocation, so a vector access of the shifted side would show in its guards
    or values): mixed congruence falls back to the element path."""
    for off in range(1, 8):
        lead = [0, 0, 0, 0]
        lead[which] = off
        run_case([40, 8192 + 24, 7], mode, side, lead=tuple(lead), own=True, first=lambda i: i == 2,
                 coef=COEF if off % 2 else None, write_clipped=off == 3)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("mode", MODES)
def test_views_at_element_alignment(mode, side):
    """Views into one allocation whose element offsets run through the residues (lead 1, gaps
    1 / 2 / 3): nothing next to a tensor is touched."""
    for gap in (1, 2, 3):
        run_case(BASE, mode, side, lead=(1, 1, 1, 1), gap=gap)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("mode", MODES)
def test_a_tensor_across_several_tiles(mode, side):
    run_case([100, 3 * 8192 + 5, 50], mode, side, first=lambda i: False)
    run_case([3 * 8192 + 5], mode, side, own=True, first=lambda i: True, coef=COEF)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("count", [CAP - 1, CAP, CAP + 1])
def test_chunk_boundaries_inside_a_tile(count, side):
    lens = [1 + i % 13 for i in range(count)]
    assert run_case(lens, "mixed", side) == -(-count // CAP)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("mode", MODES)
def test_zero_length_and_no_grad_tensors(mode, side):
    run_case([0, 5, 0, 0, 4100, 0], mode, side)
    # a tensor without a gradient between two updated ones: packed (plain) or passed over (master)
    run_case([300, 8195, 40, 9000, 7], mode, side, nograd=(1, 2))
    run_case([300, 8195, 40], mode, side, nograd=(1,), write=False, coef=COEF)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("mode", MODES)
def test_flat_alignment_and_no_flat(mode, side):
    run_case(BASE, mode, side, flat_shift=1)  # flat / master at 4-byte alignment: elementwise
    if side == "plain":
        run_case(BASE, mode, side, flat_shift=None)  # no flat side: params only
        run_case([8192 * 2 + 8, 30, 64], mode, side, flat_shift=None, own=True, nograd=(1,), coef=COEF,
                 write_clipped=True)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("mode", MODES)
def test_write_off_leaves_params_and_grads_alone(mode, side):
    """run_case compares whole storages: with write off the params must come back
    bit-identical, and the grads always do unless write_clipped."""
    run_case(BASE, mode, side, write=False)
    run_case([8192 + 16, 64], mode, side, write=False, own=True, coef=COEF)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_uniform_hyperparameter_sets(mode, side):
    """AdamW's and Adam's decay and none, both branches of the lerp, the first step and a late
    one, with and without the clip coefficient."""
    for wd, dec in [(0.01, True), (1e-4, False), (0.0, False)]:
        for b1 in (0.9, 0.4):
            for fst, step in ((True, 1), (False, 1000)):
                run_case([33, 8195], mode, side, hp=lambda i: (3e-4, b1, 0.999, 1e-8, wd, step, dec),
                         first=lambda i: fst, coef=COEF if fst else None)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_special_values(mode, side):
    """+-0, +-inf, NaN, denormals and values that overflow fp16 (SPECIAL, sprinkled by _values
    into p, g, m and v), moments over the whole exponent range, and eps = 0 on a v that holds
    zeros: 0 / 0 is NaN on both sides."""
    run_case([4099, 70], mode, side, first=lambda i: False, m_range=(-30, 30), v_range=(-38, 30))
    run_case([4099, 70], mode, side, first=lambda i: False, coef=COEF, write_clipped=True, v_range=(-45, -20),
             hp=lambda i: (1e-3, 0.9 if i else 0.4, 0.999, 0.0, 0.01, 3, i == 0))
    # v = 0 everywhere it is read, m = 0 with it on the first step, eps = 0
    from chocosgd_amd import codec
    dt = DTYPES[mode]
    m = 8192 + 9
    p = torch.from_numpy(_values(m, 1, -3, 1)).to(DEV).to(dt)
    g = torch.from_numpy(_values(m, 2, -4, 0)).to(DEV).to(dt)
    g[::3] = 0
    mdt = torch.float32 if side == "master" else dt
    ea, es = torch.zeros(m, device=DEV, dtype=mdt), torch.zeros(m, device=DEV, dtype=mdt)
    x = p.float().clone()
    pw, gw = host(p), host(g)
    if side == "master":
        want = AO.adam_master_step(pw, gw, None, None, 1e-3, eps=0.0, step=2, first=True, dtype=mode)
        codec.params_adam_master([p], [g], [ea], [es], 1e-3, eps=0.0, step=2, master=x)
        assert same_bits(host(x), want[0]) and same_bits(host(p), want[3])
    else:
        want = AO.adam_step(pw, gw, None, None, 1e-3, eps=0.0, step=2, first=True, dtype=mode)
        codec.params_adam([p], [g], [ea], [es], 1e-3, eps=0.0, step=2, flat=x)
        assert same_bits(host(x), want[0]) and same_bits(host(p), want[0])
    assert same_bits(host(ea), want[1]) and same_bits(host(es), want[2])
    assert np.isnan(want[0][::3]).all() and np.isfinite(want[0]).any(), "0 / 0 where g, and so m and v, are zero"


def test_python_entry_points_refuse_what_the_kernel_cannot_take():
    from chocosgd_amd import codec
    p, g, m, v = (torch.zeros(8, device=DEV) for _ in range(4))
    with pytest.raises(RuntimeError):  # a gradient of another dtype
        codec.params_adam([p], [g.half()], [m], [v], 1e-3)
    with pytest.raises(RuntimeError):  # a moment of another dtype
        codec.params_adam([p], [g], [m.half()], [v], 1e-3)
    with pytest.raises(RuntimeError):  # a 16-bit moment under a master update
        codec.params_adam_master([p.half()], [g.half()], [m.half()], [v], 1e-3, master=torch.zeros(8, device=DEV))
    with pytest.raises(RuntimeError):  # flat of the wrong length
        codec.params_adam([p], [g], [m], [v], 1e-3, flat=torch.zeros(9, device=DEV))
    with pytest.raises(RuntimeError, match="betas"):
        codec.params_adam([p], [g], [m], [v], 1e-3, betas=(1.0, 0.999))
    with pytest.raises(RuntimeError, match="write_clipped"):
        codec.params_adam([p], [g], [m], [v], 1e-3, write_clipped=True)
    with pytest.raises(RuntimeError):  # CPU tensors
        codec.params_adam([p.cpu()], [g.cpu()], [m.cpu()], [v.cpu()], 1e-3)


# ----------------------------------------------------------------------------- apply_adam
def _finite(m, seed, lo, hi):
    """_values without the special ones: a total gradient norm must stay finite."""
    rng = np.random.RandomState(seed)
    return (rng.standard_normal(m) * 10.0 ** rng.uniform(lo, hi, m)).astype(np.float32)


def _model(lens, mode, seed=5):
    dts = _dtypes(mode, len(lens))
    params = [torch.nn.Parameter(torch.from_numpy(_finite(m, seed + i, -2, 0)).to(DEV).to(dt))
              for i, (m, dt) in enumerate(zip(lens, dts))]
    groups = []
    for i, p in enumerate(params):
        lr, b1, b2, eps, wd, _, dec = _varied_hp(i)
        groups.append({"params": [p], "name": f"p{i}", "lr": lr, "betas": (b1, b2), "eps": eps, "weight_decay": wd,
                       "decoupled_weight_decay": dec, "amsgrad": False, "maximize": False, "capturable": False,
                       "differentiable": False, "foreach": None, "fused": None})
    return params, groups, dts


def _grads(params, step, nograd=()):
    for i, p in enumerate(params):
        p.grad = None if i in nograd else torch.from_numpy(_finite(p.numel(), 100 * step + i, -3, -1)).to(DEV).to(p.dtype)


@pytest.mark.parametrize("clip", [None, 0.05])
@pytest.mark.parametrize("side", SIDES)
def test_three_steps_through_apply_adam(side, clip):
    """A small mixed model, one tensor without a gradient, three steps: params, moments, step
    counts, the flat output / the master copy, and the launches -- params_adam_launches(k) of
    the update per step (plus the norm pass's own when clipping) and no pack."""
    from chocosgd_amd import codec, utils
    lens = [5, 8200, 33, 4097, 64, 1]
    nograd = (2,)
    params, groups, dts = _model(lens, "mixed")
    names = [(i, f"p{i}") for i in range(len(lens))]
    master = side == "master"
    mw = utils.MasterWeights(groups, names) if master else None
    flat = None if master else torch.full((sum(lens),), SENTINEL, device=DEV)
    state = collections.defaultdict(dict)
    x = [host(p) for p in params]  # the fp32 trajectory (master) / the params (plain)
    x0 = [a.copy() for a in x]
    mom = [(None, None)] * len(lens)
    for k in range(3):
        _grads(params, k, nograd)
        c0 = _counts()
        utils.apply_adam(groups, state, flat_out=flat, master=mw, clip_norm=clip)
        c1 = _counts()
        want = [0, codec.params_adam_launches(len(lens)), 0] if master else [codec.params_adam_launches(len(lens)), 0, 0]
        assert [b - a for a, b in zip(c0, c1)] == want
        coef = None
        if clip is not None:  # the coefficient the norm pass left on the device (test_gpu_gclip.py pins it)
            coef = float(utils._adam_plan(params).sgd._gn_out[1])
            assert 0.0 < coef < 1.0, "the clip must bite"
        for i, (p, gr) in enumerate(zip(params, groups)):
            if i in nograd:
                assert p not in state
                continue
            a = (gr["lr"], gr["betas"][0], gr["betas"][1], gr["eps"], gr["weight_decay"], k + 1,
                 gr["decoupled_weight_decay"], k == 0, coef)
            if master:
                x[i], m_new, v_new, p_want, _ = AO.adam_master_step(x[i], host(p.grad), *mom[i], *a, dtype=NAMES[dts[i]])
            else:
                x[i], m_new, v_new, _ = AO.adam_step(x[i], host(p.grad), *mom[i], *a, dtype=NAMES[dts[i]])
                p_want = x[i]
            mom[i] = (m_new, v_new)
            assert same_bits(host(p), p_want), (k, i, "p")
            assert same_bits(host(state[p]["exp_avg"]), m_new) and same_bits(host(state[p]["exp_avg_sq"]), v_new), (k, i)
            assert state[p]["exp_avg"].dtype == (torch.float32 if master else p.dtype)
            assert float(state[p]["step"]) == k + 1 and not state[p]["step"].is_cuda
        assert same_bits(host(mw.buffer if master else flat), np.concatenate(x)), (k, "flat / master")
    assert not same_bits(x[1], x0[1]) and same_bits(x[2], x0[2]), "the params moved, but for the one without a gradient"


def test_apply_adam_falls_back_to_the_loop_with_the_same_bits():
    """A non-contiguous gradient: the per-tensor loop runs (no launch of the kernel), and fp32
    results are the kernel's."""
    from chocosgd_amd import utils
    p0, g0 = _values(600, 3, -3, 1), _values(600, 4, -4, 0)
    got = []
    for contiguous in (True, False):
        p = torch.nn.Parameter(torch.from_numpy(p0).to(DEV).view(20, 30))
        g = torch.from_numpy(g0).to(DEV).view(20, 30)
        p.grad = g if contiguous else g.t().contiguous().t()
        groups = [{"params": [p], "lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.01,
                   "decoupled_weight_decay": True}]
        state = collections.defaultdict(dict)
        c0 = _counts()
        flat = torch.empty(600, device=DEV)
        for _ in range(2):
            utils.apply_adam(groups, state, flat_out=flat)
        assert _counts()[0] - c0[0] == (2 if contiguous else 0)
        assert same_bits(host(flat), host(p).reshape(-1))
        got.append((host(p).reshape(-1), host(state[p]["exp_avg"]).reshape(-1), host(state[p]["exp_avg_sq"]).reshape(-1)))
    want = (p0, None, None)
    for k in range(2):
        want = AO.adam_step(want[0], g0, want[1], want[2], 1e-3, wd=0.01, step=k + 1, decoupled=True, first=k == 0)[:3]
    assert all(same_bits(a, b) for a, b in zip(got[0], want)), "the kernel"
    # the loop on the device: torch's ROCm kernels divide by a host scalar with a reciprocal
    # multiply and contract as they please, so the loop's bits are pinned on CPU tensors only
    # (test_adam_host.py); here it must be the same update to a few ulps
    finite = np.isfinite(want[0])
    assert finite.sum() > 500 and all(np.allclose(a[finite], b[finite], rtol=1e-5, atol=1e-30)
                                      for a, b in zip(got[1], want))


# ----------------------------------------------------------------------------- the drop-in
def _dropin_run(op, master, fused, clip):
    """ResNet-20's layout, three CHOCO steps on one rank looped back on itself, a bf16 model.
    fused: fused_step(state=, update="adam"), with or without master weights; not fused:
    apply_adam and then today's fused_step(state=None) -- with master on the fp32 model of the
    same (widened) parameters and gradients, the trajectory master weights follow."""
    from chocosgd_amd import utils
    from chocosgd_amd.parallel_choco import CHOCOCompressor
    from chocosgd_amd.tensor_buffer import TensorBuffer
    lens = golden_json("layouts.json")["resnet20_cifar10"]
    n = sum(lens)
    dtype = torch.float32 if (master and not fused) else torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(7)
    init = [torch.randn(m, generator=g, device=DEV).to(torch.bfloat16) for m in lens]
    params = [torch.nn.Parameter(t.to(dtype)) for t in init]
    groups = [{"params": [p], "name": f"p{i}", "lr": 1e-2, "betas": (0.9, 0.999), "eps": 1e-8,
               "weight_decay": 0.0 if i % 3 == 1 else 0.01, "decoupled_weight_decay": i % 2 == 0}
              for i, p in enumerate(params)]
    names = list(enumerate(gr["name"] for gr in groups))
    shapes = [(torch.Size([m]), m) for m in lens]
    sizes = [(m,) for m in lens]
    hat = torch.cat([p.detach().float() for p in params]) + 0.1 * torch.randn(n, generator=g, device=DEV)
    mem = hat + 0.05 * torch.randn(n, generator=g, device=DEV)
    nhp = {0: TensorBuffer.from_flat(hat, sizes), "memory": TensorBuffer.from_flat(mem, sizes)}
    comp = CHOCOCompressor(aggregator=PS._Loopback(), comm_op=op, comm_device="gpu", compress_ratio=0.9,
                           quantize_level=4, is_biased=False, backend="nccl", use_ipc=False)
    state = collections.defaultdict(dict)
    mw = utils.MasterWeights(groups, names) if (master and fused) else None
    torch.manual_seed(1234)
    out = []
    for step in range(3):
        for i, p in enumerate(params):
            gg = torch.Generator(device=DEV).manual_seed(1000 * step + i)
            p.grad = (0.1 * torch.randn(p.shape, generator=gg, device=DEV)).to(torch.bfloat16).to(dtype)
        c0 = _counts()
        if fused:
            sb = utils.fused_step(comp, groups, names, shapes, nhp, {0: 1.0}, PS.GAMMA, 0, state=state, master=mw,
                                  clip_norm=clip, update="adam")
            want = [0, -(-len(lens) // CAP), 0] if mw is not None else [-(-len(lens) // CAP), 0, 0]
            assert [b - a for a, b in zip(c0, _counts())] == want, "the update's launches, and no pack"
        else:
            utils.apply_adam(groups, state, clip_norm=clip)
            sb = utils.fused_step(comp, groups, names, shapes, nhp, {0: 1.0}, PS.GAMMA, 0)
        x = host(mw.buffer) if mw is not None else PS._cat(params)
        if mw is not None:
            assert same_bits(PS._cat(params), SO.to_grid(x, "bf16")), "params = narrow(master)"
        out.append({"x": x, "msg": PS._MESSAGE[op](sb).contiguous().view(torch.uint8).cpu().numpy().copy(),
                    "hat": host(nhp[0].buffer), "mem": host(nhp["memory"].buffer),
                    "m": PS._cat([state[p]["exp_avg"] for p in params]),
                    "v": PS._cat([state[p]["exp_avg_sq"] for p in params])})
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("clip", [None, 0.5])
@pytest.mark.parametrize("master", [False, True])
@pytest.mark.parametrize("op", ["compress_top_k", "sign"])
def test_fused_step_with_adam_is_apply_adam_then_todays_step(op, master, clip):
    a = _dropin_run(op, master, True, clip)
    b = _dropin_run(op, master, False, clip)
    for step, (ra, rb) in enumerate(zip(a, b)):
        assert ra.keys() == rb.keys()
        for key in ra:
            if key == "msg":
                assert ra[key].size > 0 and np.array_equal(ra[key], rb[key]), (step, key)
            else:
                assert same_bits(ra[key], rb[key]), (step, key)
    assert not same_bits(a[0]["x"], a[1]["x"]), "the params did not move"
