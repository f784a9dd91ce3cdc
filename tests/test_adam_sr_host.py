"""Stochastic rounding for bf16 Adam, host side (no GPU): the lanes of the bit stream
(chocosgd_amd/rounding.py against include/choco_codec.h's definition, restated a second time in
tests/_adam_sr_oracle.py), utils.apply_adam_sr_loop on CPU tensors against the restatement bit
for bit, the two experiments that motivate the feature (the second moment decays, small updates
survive), the refusals, the state's round trip through torch.optim.AdamW and the argument
checks of choco_params_adam_sr, made before any HIP call."""
import collections
import copy
import ctypes

import numpy as np
import pytest
import torch

from conftest import same_bits
import _adam_oracle as AO
import _adam_sr_oracle as ASO
from chocosgd_amd import _lib, codec, utils

BF16, F32 = torch.bfloat16, torch.float32
NAMES = {BF16: "bf16", F32: "fp32"}
# the seeds and steps tests/test_sr_host.py draws with
STREAMS = [(0, 0), (5, 3), (2 ** 64 - 1, 2 ** 40 + 7), (11, 0), (9, 4)]


# ----------------------------------------------------------------------------- lanes
@pytest.mark.parametrize("seed,step", STREAMS)
def test_lane_zero_is_the_stream_every_caller_has(seed, step):
    for start, n in [(0, 41), (3, 8190), (8191, 9), (2 ** 31 - 5, 5)]:
        assert np.array_equal(utils.sr_bits(seed, step, start, n), utils.sr_bits(seed, step, start, n, lane=0))
        assert np.array_equal(utils.sr_bits(seed, step, start, n), utils.sr_bits(seed, step, start, n, 0))


@pytest.mark.parametrize("seed,step", STREAMS)
def test_lanes_follow_the_header_definition(seed, step):
    """Against the restatement in Python integers (tests/_adam_sr_oracle.py)."""
    for lane in range(3):
        for start, n in [(0, 41), (4093, 300)]:
            got = utils.sr_bits(seed, step, start, n, lane=lane)
            assert got.dtype == np.uint16
            assert np.array_equal(got.astype(np.uint32), ASO.bits16(seed, step, start, n, lane)), (lane, start)
    with pytest.raises(RuntimeError):
        utils.sr_bits(seed, step, 0, 4, lane=-1)


def test_lanes_differ_and_do_not_depend_on_start():
    lanes = [utils.sr_bits(5, 3, 0, 10_000, lane=lane) for lane in range(3)]
    for a in range(3):
        for b in range(a + 1, 3):
            # independent 16-bit draws agree in about 10000 / 65536 places
            assert int((lanes[a] == lanes[b]).sum()) <= 4, (a, b)
        for start, n in [(0, 1), (1, 7), (3, 8190), (8191, 9), (4093, 5000), (9999, 1), (17, 0)]:
            assert np.array_equal(utils.sr_bits(5, 3, start, n, lane=a), lanes[a][start:start + n]), (a, start, n)


@pytest.mark.parametrize("seed,step", [(5, 3), (11, 0)])
def test_each_lane_is_uniform_and_the_lanes_are_uncorrelated(seed, step):
    """65,536 consecutive elements: a uniform 16-bit field has mean 65535 / 2 and standard
    deviation 65536 / sqrt(12) = 18,918, so the mean of 65,536 draws has standard error
    18,918 / 256 = 73.9 and the sample correlation of two independent lanes 1 / 256; the bounds
    are six of each."""
    n = 65536
    lanes = [utils.sr_bits(seed, step, 0, n, lane=lane).astype(np.float64) for lane in range(3)]
    for lane, x in enumerate(lanes):
        print(f"lane {lane}: mean {x.mean():.1f}")
        assert abs(x.mean() - 65535 / 2) <= 6 * 18918 / 256, (lane, x.mean())
    for a in range(3):
        for b in range(a + 1, 3):
            r = float(np.corrcoef(lanes[a], lanes[b])[0, 1])
            print(f"lanes {a}, {b}: correlation {r:+.5f}")
            assert abs(r) < 6 / 256, (a, b, r)


# ----------------------------------------------------------------------------- the loop against the restatement
LENS = [5, 4099, 33, 1, 260, 2051]
DTYPES = [BF16, F32, BF16, BF16, F32, BF16]
NOGRAD = (2,)
SEED = 5
PINNED_TOTAL = 20.0  # about the gradients' norm: the coefficient bites, and is the same number on both sides
CONFIGS = {"adamw": (0.01, True), "adam": (1e-4, False), "nowd": (0.0, False)}


def _model(dtypes=DTYPES, wd=0.01, decoupled=True, beta1=0.9, seed=3):
    rng = np.random.RandomState(seed)
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(m).astype(np.float32)).to(dt))
              for m, dt in zip(LENS, dtypes)]
    groups = [{"params": [p], "lr": 1e-3 * (1 + i), "betas": (beta1, 0.999), "eps": 1e-8, "weight_decay": wd,
               "decoupled_weight_decay": decoupled, "amsgrad": False, "maximize": False, "foreach": None,
               "capturable": False, "differentiable": False, "fused": None} for i, p in enumerate(params)]
    return params, groups


def _set_grads(params, step, nograd=NOGRAD):
    rng = np.random.RandomState(100 + step)
    for i, p in enumerate(params):
        g = torch.from_numpy((0.1 * rng.standard_normal(p.numel())).astype(np.float32)).to(p.dtype)
        p.grad = None if i in nograd else g


def _np(t):
    return t.detach().float().numpy().copy()


def _coef(total, max_norm):
    """clip_grads_with_norm_'s lines in fp32: min(1, max_norm * (1 / (total + 1e-6)))."""
    f = np.float32
    return float(min(f(f(f(1) / f(f(total) + f(1e-6))) * f(max_norm)), f(1)))


@pytest.mark.parametrize("via", ["apply_adam", "loop"])
@pytest.mark.parametrize("clip", [None, 0.5])
@pytest.mark.parametrize("beta1", [0.9, 0.4])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_cpu_loop_is_the_restatement(name, beta1, clip, via):
    """Three steps (FIRST, then warm) of a mixed bf16 / fp32 model with one tensor without a
    gradient, flat_out given: parameters, moments, flat and the gradients against
    _adam_sr_oracle, bit for bit; the fp32 tensors against plain apply_adam on a twin model."""
    wd, decoupled = CONFIGS[name]
    params, groups = _model(wd=wd, decoupled=decoupled, beta1=beta1)
    twins, twin_groups = _model(wd=wd, decoupled=decoupled, beta1=beta1)
    state, twin_state = collections.defaultdict(dict), collections.defaultdict(dict)
    flat = torch.full((sum(LENS),), -7.0)
    want = [(_np(p), None, None) for p in params]
    coef = None if clip is None else _coef(PINNED_TOTAL, clip)
    assert coef is None or 0.0 < coef < 1.0
    kw = {} if clip is None else dict(clip_norm=clip, total_norm=PINNED_TOTAL)
    for k in range(3):
        _set_grads(params, k)
        _set_grads(twins, k)
        grads = [None if p.grad is None else _np(p.grad) for p in params]
        if via == "apply_adam":
            utils.apply_adam(groups, state, flat_out=flat, rounding=(SEED, 7 + k), **kw)
        else:
            utils.apply_adam_sr_loop(groups, state, SEED, 7 + k, None if clip is None else (clip, False, PINNED_TOTAL),
                                     flat)
        utils.apply_adam(twin_groups, twin_state, **kw)
        off, flats = 0, []
        for i, (p, gr) in enumerate(zip(params, groups)):
            if grads[i] is None:
                assert p not in state and same_bits(_np(p), want[i][0])
                flats.append(want[i][0])
                off += LENS[i]
                continue
            pw, mw, vw = want[i]
            out = ASO.adam_sr_step(pw, grads[i], mw, vw, gr["lr"], gr["betas"][0], gr["betas"][1], gr["eps"],
                                   gr["weight_decay"], k + 1, gr["decoupled_weight_decay"], first=k == 0, coef=coef,
                                   dtype=NAMES[p.dtype], seed=SEED, sr_step=7 + k, start=off)
            want[i] = out[:3]
            flats.append(out[4])
            assert same_bits(_np(p), out[0]), (k, i, "p")
            assert same_bits(_np(state[p]["exp_avg"]), out[1]), (k, i, "exp_avg")
            assert same_bits(_np(state[p]["exp_avg_sq"]), out[2]), (k, i, "exp_avg_sq")
            assert state[p]["exp_avg"].dtype == p.dtype and state[p]["exp_avg_sq"].dtype == p.dtype
            assert same_bits(_np(p.grad), grads[i]), "the gradient was written"
            assert float(state[p]["step"]) == k + 1 and not state[p]["step"].is_cuda
            if p.dtype == F32:
                t = twins[i]
                assert same_bits(_np(p), _np(t)) and same_bits(_np(state[p]["exp_avg"]), _np(twin_state[t]["exp_avg"]))
                assert same_bits(_np(state[p]["exp_avg_sq"]), _np(twin_state[t]["exp_avg_sq"]))
            else:
                assert float(((out[4].view(np.uint32) & 0xFFFF) != 0).mean()) > 0.5, "flat is unrounded"
            off += LENS[i]
        assert same_bits(flat.numpy(), np.concatenate(flats)), (k, "flat")


def test_cpu_loop_write_off_and_write_clipped():
    """write=False leaves the parameters alone and still rounds the moments; write_clipped stores
    c * g, rounded to nearest in a bf16 gradient."""
    params, groups = _model()
    _set_grads(params, 0)
    before = [_np(p) for p in params]
    grads = [None if p.grad is None else _np(p.grad) for p in params]
    state = collections.defaultdict(dict)
    flat = torch.empty(sum(LENS))
    coef = _coef(PINNED_TOTAL, 0.5)
    utils.apply_adam_sr_loop(groups, state, SEED, 0, (0.5, True, PINNED_TOTAL), flat, write=False)
    off = 0
    for i, (p, gr) in enumerate(zip(params, groups)):
        assert same_bits(_np(p), before[i]), i
        if grads[i] is not None:
            out = ASO.adam_sr_step(before[i], grads[i], None, None, gr["lr"], 0.9, 0.999, 1e-8, 0.01, 1, True, first=True,
                                   coef=coef, dtype=NAMES[p.dtype], seed=SEED, sr_step=0, start=off)
            assert same_bits(_np(state[p]["exp_avg"]), out[1]) and same_bits(_np(state[p]["exp_avg_sq"]), out[2])
            assert same_bits(_np(p.grad), out[3]) and not same_bits(out[3], grads[i])
            assert same_bits(flat[off:off + LENS[i]].numpy(), out[4])
        off += LENS[i]


# ----------------------------------------------------------------------------- what it is for
def _one(n, p0, g0, lr, device="cpu"):
    p = torch.nn.Parameter(torch.full((n,), p0, dtype=BF16, device=device))
    p.grad = torch.full((n,), g0, dtype=BF16, device=device)
    groups = [{"params": [p], "lr": lr, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.0}]
    return p, groups


def second_moment_experiment(device):
    """4,096 bf16 elements, v = 1.0, m = 0, g = 0, beta2 = 0.999, 200 steps.  Returns v after
    plain apply_adam and after apply_adam(rounding=)."""
    out = []
    for rounding in (None, utils.StochasticRounding(3)):
        p, groups = _one(4096, 1.0, 0.0, 1e-4, device)
        state = collections.defaultdict(dict)
        state[p] = {"step": torch.tensor(0.0), "exp_avg": torch.zeros_like(p.data), "exp_avg_sq": torch.ones_like(p.data)}
        for _ in range(200):
            if rounding is None:
                utils.apply_adam(groups, state)
            else:
                utils.apply_adam(groups, state, rounding=rounding)
        assert rounding is None or rounding.state_dict()["step"] == 200
        assert torch.equal(p.data, torch.ones_like(p.data)) and float(state[p]["exp_avg"].abs().max()) == 0.0
        out.append(state[p]["exp_avg_sq"].detach().double().cpu())
    return out


def test_the_second_moment_decays():
    """v = rnd(v * 0.999) changes v by a relative 1e-3, below half a bf16 ulp (2^-9 just below a
    power of two): round-to-nearest returns 1.0 at every step, and the moving average never
    decays.  With rounding= the mean of v is within 1 % of 0.999^200 = 0.8186: the per-step
    rounding noise is at most ulp / 2 ~ 2^-9 relative, after 200 steps at most 2.8 % per element
    and 0.05 % on the mean of 4,096, so 1 % is more than 20 standard deviations -- and nowhere
    near the stalled 1.0."""
    plain, rounded = second_moment_experiment("cpu")
    assert torch.equal(plain, torch.ones(4096, dtype=torch.float64)), "the stall this feature is for"
    mean, want = float(rounded.mean()), 0.999 ** 200
    print(f"mean of v after 200 steps: {mean:.5f} (0.999^200 = {want:.5f})")
    assert abs(mean - want) <= 0.01 * want, mean


def small_update_experiment(device):
    """4,096 bf16 elements, p = 1.0, g = 1.0, lr = 1e-4, wd = 0, 200 steps.  Returns p after
    plain apply_adam, p after apply_adam(rounding=), and the fp32 restatement's p."""
    out = []
    for rounding in (None, utils.StochasticRounding(3)):
        p, groups = _one(4096, 1.0, 1.0, 1e-4, device)
        state = collections.defaultdict(dict)
        for _ in range(200):
            if rounding is None:
                utils.apply_adam(groups, state)
            else:
                utils.apply_adam(groups, state, rounding=rounding)
        out.append(p.detach().double().cpu())
    ref = (np.ones(1, np.float32), None, None)
    for k in range(200):
        ref = AO.adam_step(ref[0], np.ones(1, np.float32), ref[1], ref[2], 1e-4, step=k + 1, first=k == 0, dtype="fp32")[:3]
    return out[0], out[1], float(ref[0][0])


def test_small_updates_survive():
    """An Adam step moves a weight by about lr = 1e-4; at |p| ~ 1 that is a twentieth of half a
    bf16 ulp (2^-8 below 1.0), so the plain bf16 update leaves p at exactly 1.0 for ever.  With
    rounding= the mean displacement of p is within 5 % of the fp32 restatement's
    (_adam_oracle.adam_step(dtype="fp32") on the same inputs: about 200 * 1e-4 = 0.02).  The
    bound: each step moves an element one ulp (2^-8 = 3.9e-3) down with probability
    1e-4 / 3.9e-3 = 0.0256, a variance of (3.9e-3)^2 * 0.0256 * 0.974 = 3.8e-7 per step and
    7.6e-5 after 200, so sigma is 8.7e-3 per element and 8.7e-3 / 64 = 1.4e-4 on the mean of
    4,096; 5 % of 0.02 is 1e-3, about 7 sigma.  (The stochastically rounded moments add a
    relative noise of 2^-9 per step to q = m / den, far below that.)"""
    plain, rounded, ref = small_update_experiment("cpu")
    assert torch.equal(plain, torch.ones(4096, dtype=torch.float64)), "the stall this feature is for"
    moved, want = 1.0 - float(rounded.mean()), 1.0 - ref
    print(f"mean displacement after 200 steps: {moved:.6f} (fp32: {want:.6f})")
    assert 0.019 < want < 0.021
    assert abs(moved - want) <= 0.05 * want, moved


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


@pytest.mark.parametrize("warm", [False, True])
def test_refusals_raise_before_anything_changes_or_the_stream_advances(warm):
    names = [(i, f"p{i}") for i in range(len(LENS))]
    params, groups = _model()
    _set_grads(params, 0, nograd=())
    state = collections.defaultdict(dict)
    sr = utils.StochasticRounding(3)
    if warm:
        utils.apply_adam(groups, state, rounding=sr)
    at = sr.state_dict()["step"]
    snap = _snapshot(params, state)
    master = utils.MasterWeights(groups, names)
    fused = (None, groups, names, None, None, None, 0.5, 0)
    with pytest.raises(RuntimeError, match="master"):
        utils.apply_adam(groups, state, master=master, rounding=sr)
    with pytest.raises(RuntimeError, match="rounding"):
        utils.fused_step(*fused, state=state, update="adam_sr")
    with pytest.raises(RuntimeError, match="state"):
        utils.fused_step(*fused, update="adam_sr", rounding=sr)
    with pytest.raises(RuntimeError, match="loss_scale"):
        utils.fused_step(*fused, state=state, update="adam_sr", rounding=sr, loss_scale=utils.LossScaler("cpu"))
    with pytest.raises(RuntimeError, match="master"):
        utils.fused_step(*fused, state=state, update="adam_sr", rounding=sr, master=master)
    # the arithmetic of update="adam" is torch's per-line bf16: it keeps refusing rounding= and loss_scale=
    with pytest.raises(RuntimeError, match="section 8"):
        utils.fused_step(*fused, state=state, update="adam", rounding=sr)
    with pytest.raises(RuntimeError, match="section 8"):
        utils.fused_step(*fused, state=state, update="adam", loss_scale=utils.LossScaler("cpu"))
    with pytest.raises(RuntimeError, match="update"):
        utils.fused_step(*fused, state=state, update="adam-sr", rounding=sr)
    # what apply_adam refuses today, in the LAST group
    for key, val in [("amsgrad", True), ("maximize", True), ("capturable", True), ("differentiable", True),
                     ("lr", torch.tensor(1e-3))]:
        old = groups[-1].get(key)
        groups[-1][key] = val
        with pytest.raises(RuntimeError):
            utils.apply_adam(groups, state, rounding=sr)
        with pytest.raises(RuntimeError):
            utils.fused_step(*fused, state=state, update="adam_sr", rounding=sr)
        with pytest.raises(RuntimeError):
            utils.apply_adam_sr_loop(groups, state, 3, 0)
        groups[-1][key] = old
    with pytest.raises(RuntimeError, match="write_clipped"):
        utils.apply_adam(groups, state, write_clipped=True, rounding=sr)
    with pytest.raises(RuntimeError, match="flat_out"):
        utils.apply_adam(groups, state, flat_out=torch.zeros(sum(LENS) + 1), rounding=sr)
    _unchanged(params, state, snap)
    assert torch.equal(master.buffer, torch.cat([p.detach().float() for p in params]))
    assert sr.state_dict()["step"] == at


def test_fp16_parameters_and_foreign_moments_are_refused():
    names = [(i, f"p{i}") for i in range(len(LENS))]
    sr = utils.StochasticRounding(3)
    p16, g16 = _model([torch.float16] + DTYPES[1:])
    _set_grads(p16, 0, nograd=())
    state = collections.defaultdict(dict)
    snap = _snapshot(p16, state)
    fused = (None, g16, names, None, None, None, 0.5, 0)
    with pytest.raises(RuntimeError, match="float16"):
        utils.apply_adam(g16, state, rounding=sr)
    with pytest.raises(RuntimeError, match="float16"):
        utils.fused_step(*fused, state=state, update="adam_sr", rounding=sr)
    with pytest.raises(RuntimeError, match="float16"):
        utils.apply_adam_sr_loop(g16, state, 3, 0)
    _unchanged(p16, state, snap)
    # fp32 moments beside bf16 parameters (a state written under master weights)
    params, groups = _model()
    _set_grads(params, 0, nograd=())
    state = collections.defaultdict(dict)
    utils.apply_adam(groups, state, master=utils.MasterWeights(groups, names))
    assert state[params[0]]["exp_avg"].dtype == F32
    snap = _snapshot(params, state)
    fused = (None, groups, names, None, None, None, 0.5, 0)
    with pytest.raises(RuntimeError, match="moments"):
        utils.apply_adam(groups, state, rounding=sr)
    with pytest.raises(RuntimeError, match="moments"):
        utils.fused_step(*fused, state=state, update="adam_sr", rounding=sr)
    with pytest.raises(RuntimeError, match="moments"):
        utils.apply_adam_sr_loop(groups, state, 3, 0)
    _unchanged(params, state, snap)
    assert sr.state_dict()["step"] == 0


def test_steps_outside_the_feature_stay_as_they_are():
    from chocosgd_amd import dcd, deep_squeeze, dgc, ecd, ef_sign
    sr = utils.StochasticRounding(3)
    calls = [(utils.dpsgd_step, 5), (utils.allreduce_sgd_step, 4), (dcd.fused_step, 7), (ecd.fused_step, 8),
             (deep_squeeze.fused_step, 7), (ef_sign.fused_step, 5), (dgc.fused_step, 6)]
    for fn, nargs in calls:
        with pytest.raises(RuntimeError, match="rounding"):
            fn(*([None] * nargs), rounding=sr)
        with pytest.raises(TypeError):
            fn(*([None] * nargs), update="adam_sr")
    assert sr.state_dict()["step"] == 0


# ----------------------------------------------------------------------------- torch's keys
def test_state_loads_into_torch_adamw_and_back():
    """Two stochastic steps on a bf16 model, the state handed to torch.optim.AdamW through its own
    load_state_dict, a step there; then plain apply_adam and apply_adam(rounding=) continue on
    torch's state, the moments and the count taken over as they are."""
    g = torch.Generator().manual_seed(1)
    params = [torch.nn.Parameter(torch.randn(m, generator=g).to(BF16)) for m in (7, 130)]
    opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=0.01, foreach=False, fused=False)
    state = collections.defaultdict(dict)
    sr = utils.StochasticRounding(9)
    for k in range(2):
        for p in params:
            p.grad = torch.full_like(p, 0.01 * (k + 1))
        utils.apply_adam(opt.param_groups, state, rounding=sr)
    sd = opt.state_dict()
    sd["state"] = {i: {key: val.clone() for key, val in state[p].items()} for i, p in enumerate(params)}
    opt.load_state_dict(sd)
    for p in params:
        assert float(opt.state[p]["step"]) == 2 and opt.state[p]["exp_avg"].dtype == BF16
        assert torch.equal(opt.state[p]["exp_avg"], state[p]["exp_avg"])
        assert torch.equal(opt.state[p]["exp_avg_sq"], state[p]["exp_avg_sq"])
    opt.step()
    assert all(float(opt.state[p]["step"]) == 3 for p in params)
    # and back: torch's state continues under rounding=, key for key
    before = [(_np(p), _np(opt.state[p]["exp_avg"]), _np(opt.state[p]["exp_avg_sq"])) for p in params]
    utils.apply_adam(opt.param_groups, opt.state, rounding=sr)
    assert sr.state_dict()["step"] == 3
    off = 0
    for p, (p3, m3, v3) in zip(params, before):
        assert float(opt.state[p]["step"]) == 4
        want = ASO.adam_sr_step(p3, _np(p.grad), m3, v3, 1e-3, wd=0.01, step=4, decoupled=True, seed=9, sr_step=2,
                                start=off)
        assert same_bits(_np(p), want[0]) and same_bits(_np(opt.state[p]["exp_avg"]), want[1])
        assert same_bits(_np(opt.state[p]["exp_avg_sq"]), want[2])
        off += p.numel()
    utils.apply_adam(opt.param_groups, opt.state)  # the plain update takes the same state
    fresh = torch.optim.AdamW(params, lr=1e-3, weight_decay=0.01, foreach=False, fused=False)
    fresh.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert all(float(fresh.state[p]["step"]) == 5 for p in params)


# ----------------------------------------------------------------------------- the C ABI
ERR_INVALID = -1  # CHOCO_ERR_INVALID
C_F32, C_BF16, C_F16 = 0, 1, 2
WRITE_PARAMS, WRITE_CLIPPED = 2, 16


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _call(lib, dts=(C_BF16, C_F32), lens=(4, 4), n=8, mode=WRITE_PARAMS, flat=0x10000, coef=0, nseg=None, null=(),
          flags=(0, 0), step=(1.0, 1.0), m=(0x5000, 0x6000)):
    k = len(dts)
    vp = lambda vals: (ctypes.c_void_p * k)(*vals)  # noqa: E731
    f64 = lambda vals: (ctypes.c_double * k)(*vals)  # noqa: E731
    tables = {"params": vp([0x1000, 0x2000][:k]), "grads": vp([0x3000, 0x4000][:k]), "exp_avg": vp(list(m)[:k]),
              "exp_avg_sq": vp([0x7000, 0x8000][:k]), "lens": (ctypes.c_int64 * k)(*lens),
              "dtypes": (ctypes.c_int32 * k)(*dts), "lr": f64([1e-3] * k), "beta1": f64([0.9] * k),
              "beta2": f64([0.999] * k), "eps": f64([1e-8] * k), "wd": f64([0.0] * k), "step": f64(step),
              "flags": (ctypes.c_int32 * k)(*flags)}
    args = [None if name in null else t for name, t in tables.items()]
    return lib.choco_params_adam_sr(*args, k if nseg is None else nseg, ctypes.c_void_p(flat), n, mode,
                                    ctypes.c_void_p(coef), 5, 3, None)


BAD = {
    "fp16 tensor": dict(dts=(C_BF16, C_F16), msg="tensor 1: fp16"),
    "unknown mode bit": dict(mode=WRITE_PARAMS | 1, msg="unknown mode bits"),
    "another unknown mode bit": dict(mode=WRITE_PARAMS | 32, msg="unknown mode bits"),
    "write_clipped without coef": dict(mode=WRITE_PARAMS | WRITE_CLIPPED, msg="WRITE_CLIPPED needs coef"),
    "nothing to write": dict(mode=0, flat=0, msg="nothing to write"),
    "flat at 2 mod 4": dict(flat=0x10002, msg="4-byte"),
    "misaligned coef": dict(coef=0x5002, msg="coef"),
    "null params": dict(null=("params",), msg="null table"),
    "null exp_avg_sq": dict(null=("exp_avg_sq",), msg="null table"),
    "null step": dict(null=("step",), msg="null table"),
    "null moment": dict(m=(0x5000, 0), msg="null exp_avg"),
    "bf16 moment at odd byte": dict(m=(0x5001, 0x6000), msg="aligned"),
    "unknown flag bit": dict(flags=(0, 8), msg="flag"),
    "step zero": dict(step=(1.0, 0.0), msg="step"),
    "sum below n": dict(n=9, msg="add up"),
    "sum above n": dict(n=7, msg="add up"),
    "nseg zero": dict(nseg=0, msg="nseg"),
    "order: flags before fp16": dict(dts=(C_F16, C_F32), flags=(8, 0), msg="flag"),
    "order: fp16 before alignment": dict(dts=(C_F16, C_F32), m=(0x5001, 0x6000), msg="fp16"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_adam_sr_rejects_invalid_arguments(lib, case):
    kw = dict(BAD[case])
    msg = kw.pop("msg")
    before = codec.launch_count("param_adam_sr_kernel")
    assert _call(lib, **kw) == ERR_INVALID, case
    err = _lib.last_error()
    assert msg in err, (case, err)
    assert codec.launch_count("param_adam_sr_kernel") == before  # nothing was launched


def test_launch_count_is_the_adam_update_s(lib):
    assert lib.choco_params_adam_launches(54) == 1 and lib.choco_params_adam_launches(55) == 2
    assert codec.params_adam_launches(161) == 3
