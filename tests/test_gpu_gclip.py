"""Global-norm gradient clipping on the device: ParamSgdPlan.gradnorm (the total norm and the
clip coefficient), the clipped update (ParamSgdPlan.run / run_master(gclip=)) and the layers
above them (utils.clip_grad_norm_, utils.apply_gradient(clip_norm=), fused_step and dpsgd_step).

The fp32 fixtures are the reference sequence's own results (tests/golden/gclip_*.npz:
torch.nn.utils.clip_grad_norm_ then the reference's apply_gradient) and are reproduced bit for
bit with the fixture's total pinned.  Everything else is checked bit for bit against the numpy
model (tests/_gclip_oracle.py on _sgd_oracle) evaluated at the device's own total, whole
storages at a time.  The total alone has a tolerance: equal or adjacent on the coefficient
dtype's grid to float32(sqrt(sum(g.astype(float64) ** 2))) -- any-order fp64 summation of
n <= 2^31 non-negative terms is within n * 2^-53 relative of the exact sum, far inside half an
fp32 ulp, so the two can only round to the same value or to neighbours."""
import collections

import numpy as np
import pytest
import torch

from conftest import golden, golden_json, same_bits
import _gclip_oracle as GO
import _sgd_oracle as SO
import test_gpu_dgc_sgd as DG  # Views (tensors inside one storage between sentinels), host, dev
import test_gpu_param_sgd as PS  # the loopback aggregator of the drop-in tests

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = DG.DTYPES
SENTINEL = DG.SENTINEL
host, dev, Views = DG.host, DG.dev, DG.Views
SETS = ["clip", "wd", "mom", "nesterov", "damp"]
STEPS = 3
LAYOUT = [5, 1, 0, 8195, 33, 4099, 17000, 40, 1500, 1]
KERNELS = ("param_sqnorm_kernel", "param_gradnorm_total_kernel", "param_sgd_gclip_kernel",
           "param_sgd_master_gclip_kernel", "param_sgd_kernel", "param_sgd_master_kernel", "param_sqnorm_finish_kernel")


@pytest.fixture(scope="module")
def inputs():
    return golden("gclip_inputs")


def _counts():
    from chocosgd_amd import codec
    return np.array([codec.launch_count(k) for k in KERNELS])


def _split(flat, lens):
    offs = np.concatenate([[0], np.cumsum(lens)])
    return [flat[offs[i]:offs[i + 1]] for i in range(len(lens))]


def _cat(tensors):
    return np.concatenate([host(t).reshape(-1) for t in tensors])


def _values(lens, seed, dtype, scale=1.0):
    rng = np.random.RandomState(seed)
    n = int(sum(lens))
    return SO.to_grid((rng.standard_normal(n) * scale * 10.0 ** rng.uniform(-3, 0, n)).astype(np.float32), dtype)


@pytest.fixture
def totals(monkeypatch):
    """Every [total, coefficient] pair ParamSgdPlan.gradnorm leaves on the device, in call order."""
    from chocosgd_amd import codec
    seen = []
    inner = codec.ParamSgdPlan.gradnorm

    def recording(self, *args, **kwargs):
        out = inner(self, *args, **kwargs)
        seen.append(host(out.clone()))
        return out

    monkeypatch.setattr(codec.ParamSgdPlan, "gradnorm", recording)
    return seen


def _check_total(got, grads, cd):
    """got = [total, c] of the device against the fp64 value: within 1 ulp of CD's grid."""
    want = GO.total(grads, cd)
    assert np.isfinite(got[0]) and got[0] >= 0
    assert same_bits(got[:1], SO.to_grid(got[:1], cd)), "a total off its dtype's grid"
    assert GO.ulp_distance(got[0], want, cd) <= 1, (got, want)


# ----------------------------------------------------------------------------- the total norm and the coefficient
def _gradnorm(g, lens, dtype, max_norm, shift=0, nograd=(), coef_dtype=None):
    """Two calls over views inside one storage; returns ([total, c], norms) of the first."""
    from chocosgd_amd import codec
    gv = Views(g, lens, dtype, shift)
    before = gv.all()
    grads = [None if s in nograd else v for s, v in enumerate(gv.views)]
    plan = codec.ParamSgdPlan(gv.views)
    for i, v in enumerate(grads):
        plan.grad_ptrs[i] = None if v is None else v.data_ptr()
        plan.flags[i] = codec.SGD_F_NOGRAD if v is None else 0
    norms = torch.full((len(lens),), SENTINEL, device=DEV)
    c0 = _counts()
    a = host(plan.gradnorm(max_norm, coef_dtype=coef_dtype, norms=norms).clone())
    na = host(norms)
    b = host(plan.gradnorm(max_norm, coef_dtype=coef_dtype, norms=norms).clone())
    d = (_counts() - c0).tolist()
    assert d[1] == 2 and d[0] + d[1] == 2 * codec.params_gradnorm_launches(len(lens)) and sum(d[2:]) == 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "two calls, two results"
    assert np.array_equal(na.view(np.uint32), host(norms).view(np.uint32))
    assert same_bits(gv.all(), before), "the norm pass wrote something"
    # the per-tensor norms are choco_params_sqnorm's at zero weight decay, bit for bit
    want = host(codec.params_sqnorm(gv.views, grads, 0.0))
    assert np.array_equal(na.view(np.uint32), want.view(np.uint32)), (na, want)
    return a, na


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_total_norm_views_inside_one_storage(dtype, shift):
    g = _values(LAYOUT, 21, dtype)
    for max_norm in (0.4, 1e3):
        got, _ = _gradnorm(g, LAYOUT, dtype, max_norm, shift)
        _check_total(got, _split(g, LAYOUT), dtype)
        assert same_bits(got[1:], [GO.coef(got[0], max_norm, dtype)]), (got, max_norm)
    assert GO.coef(got[0], 0.4, dtype) < 1 and GO.coef(got[0], 1e3, dtype) == 1
    # a 16-bit layout with the coefficient asked for in fp32 (the master path)
    if dtype != "fp32":
        got, _ = _gradnorm(g, LAYOUT, dtype, 0.4, shift, coef_dtype=torch.float32)
        _check_total(got, _split(g, LAYOUT), "fp32")
        assert same_bits(got[1:], [GO.coef(got[0], 0.4, "fp32")])


def test_total_norm_of_many_small_tensors():
    """300 tensors of 1-40 elements: three chunks of the norm pass, most of them in one tile."""
    rng = np.random.RandomState(5)
    lens = rng.randint(1, 41, 300).tolist()
    g = _values(lens, 6, "fp32")
    got, _ = _gradnorm(g, lens, "fp32", 0.25)
    _check_total(got, _split(g, lens), "fp32")
    assert same_bits(got[1:], [GO.coef(got[0], 0.25)])


def test_total_norm_of_more_tensors_than_the_total_launch_stages():
    """1100 tensors: past the 1024 whose slots and meta words the total launch stages in LDS, so
    it reads the workspace in place -- the same additions in the same order."""
    rng = np.random.RandomState(8)
    lens = rng.randint(1, 9, 1100).tolist()
    g = _values(lens, 9, "fp32")
    got, _ = _gradnorm(g, lens, "fp32", 0.25)
    _check_total(got, _split(g, lens), "fp32")
    assert same_bits(got[1:], [GO.coef(got[0], 0.25)])


def test_total_norm_mixed_dtypes_default_to_an_fp32_coefficient():
    from chocosgd_amd import codec
    lens = [700, 9000, 33]
    dts = ["bf16", "fp32", "fp16"]
    gs = [_values([m], 30 + i, dt) for i, (m, dt) in enumerate(zip(lens, dts))]
    views = [dev(g, DTYPES[dt]) for g, dt in zip(gs, dts)]
    plan = codec.ParamSgdPlan(views)
    for i, v in enumerate(views):
        plan.grad_ptrs[i], plan.flags[i] = v.data_ptr(), 0
    got = host(plan.gradnorm(0.4).clone())
    _check_total(got, gs, "fp32")
    assert same_bits(got[1:], [GO.coef(got[0], 0.4, "fp32")])


def test_total_norm_does_not_overflow_where_fp32_accumulation_does():
    lens = [3000, 7]
    g = np.full(sum(lens), 1e30, dtype=np.float32)  # squares past fp32's range
    got, norms = _gradnorm(g, lens, "fp32", 0.4)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(norms))
    _check_total(got, _split(g, lens), "fp32")
    assert same_bits(got[1:], [GO.coef(got[0], 0.4)]) and 0 < got[1] < 1e-30


def test_total_norm_of_zero_gradients_and_of_no_grad_tensors():
    lens = [10, 20, 5]
    got, _ = _gradnorm(np.zeros(sum(lens), np.float32), lens, "fp32", 0.4)
    assert same_bits(got, [0.0, 1.0])
    g = _values(lens, 3, "fp32")
    got, norms = _gradnorm(g, lens, "fp32", 0.4, nograd=(1,))
    assert norms[1] == 0
    _check_total(got, [g[:10], None, g[30:]], "fp32")
    big = g.copy()
    big[10:30] = 1e30  # what the no-grad tensor would hold: it must not be read
    again, _ = _gradnorm(big, lens, "fp32", 0.4, nograd=(1,))
    assert same_bits(again, got)


# ----------------------------------------------------------------------------- pinned parity with the reference
def _device_model(p0, lens, hp, dtype="fp32"):
    lr, wd, mom, damp, nest = hp
    params = [torch.nn.Parameter(dev(v, DTYPES[dtype])) for v in _split(p0, lens)]
    groups = [{"params": [p], "name": f"p{i}", "lr": lr, "weight_decay": wd, "momentum": mom, "dampening": damp,
               "nesterov": bool(nest)} for i, p in enumerate(params)]
    return params, groups


def _set_grads(params, flat, lens):
    for p, v in zip(params, _split(flat, lens)):
        p.grad = dev(v, p.dtype)


@pytest.mark.parametrize("variant", ["plain", "flat", "write_clipped"])
@pytest.mark.parametrize("name", SETS)
def test_pinned_steps_reproduce_the_reference_fixtures(inputs, name, variant):
    """clip_grad_norm_ then the reference's apply_gradient, three steps, through
    utils.apply_gradient(clip_norm=, total_norm=<the total torch returned>)."""
    from chocosgd_amd import codec, utils
    fx = golden(f"gclip_{name}")
    hp = fx["hp"].tolist()
    lens = inputs["lens"].tolist()
    n = sum(lens)
    params, groups = _device_model(inputs["p0"], lens, hp)
    state = collections.defaultdict(dict)
    big = torch.full((n + 8,), SENTINEL, device=DEV)
    flat = big[4:4 + n] if variant == "flat" else None
    c0 = _counts()
    for k in range(STEPS):
        _set_grads(params, inputs[f"g{k}"], lens)
        grads = [p.grad for p in params]
        utils.apply_gradient(groups, state, flat_out=flat, clip_norm=float(inputs["max_norm"]),
                             write_clipped=variant == "write_clipped", total_norm=dev(fx[f"total{k}"].reshape(1)))
        assert same_bits(_cat(params), fx[f"p{k}"]), f"params after step {k}"
        if hp[2] != 0:
            assert same_bits(_cat([state[p]["momentum_buffer"] for p in params]), fx[f"buf{k}"]), f"buf, step {k}"
        assert same_bits(_cat(grads), fx[f"gc{k}"] if variant == "write_clipped" else inputs[f"g{k}"])
        assert all(p.grad is g for p, g in zip(params, grads))
        if flat is not None:
            assert same_bits(host(flat), fx[f"p{k}"]), f"flat after step {k}"
        assert torch.all(big[:4] == SENTINEL) and torch.all(big[4 + n:] == SENTINEL)
    want = np.zeros(len(KERNELS), dtype=np.int64)
    want[1] = STEPS * codec.params_gradnorm_launches(len(lens), pinned=True)
    want[2] = STEPS * codec.params_sgd_launches(len(lens))
    assert (_counts() - c0).tolist() == want.tolist()


def test_one_element_fixture_has_no_shortcut(inputs, totals):
    """g = 1, max_norm = 1: the device's total is exactly 1 and the gradient is still scaled."""
    from chocosgd_amd import utils
    params, groups = _device_model(inputs["one_p0"], [1], (float(inputs["one_lr"]), 0.0, 0.0, 0.0, False))
    _set_grads(params, inputs["one_g"], [1])
    utils.apply_gradient(groups, collections.defaultdict(dict), clip_norm=float(inputs["one_max_norm"]),
                         write_clipped=True)
    assert same_bits(totals[-1][:1], inputs["one_total"].reshape(1)) and totals[-1][1] < 1
    assert same_bits(_cat(params), inputs["one_p"]) and same_bits(_cat([params[0].grad]), inputs["one_gc"])


# ----------------------------------------------------------------------------- unpinned: the model at the device's total
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("apply_mode", [True, False], ids=["apply", "grad"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_unpinned_steps_match_the_model_at_the_device_total(inputs, totals, dtype, apply_mode, shift):
    """Norm pass, coefficient and update; parameters and gradients are views inside one storage
    each, at a shift that takes the 16-byte path (0) or the element path (1)."""
    from chocosgd_amd import codec, utils
    hp = (0.1, 5e-4, 0.9, 0.0, True)
    lens = LAYOUT
    n = sum(lens)
    p = SO.to_grid(inputs["p0"], dtype)
    pv = Views(p, lens, dtype, shift)
    params = [torch.nn.Parameter(v) for v in pv.views]
    groups = [{"params": [q], "lr": hp[0], "weight_decay": hp[1], "momentum": hp[2], "dampening": hp[3],
               "nesterov": hp[4]} for q in params]
    # the momentum buffers exist already (zeros), as views too: all three sides share the grid
    buf = np.zeros(n, dtype=np.float32)
    bv = Views(buf, lens, dtype, shift)
    state = collections.defaultdict(dict)
    for q, v in zip(params, bv.views):
        state[q]["momentum_buffer"] = v
    big = torch.full((n + 8,), SENTINEL, device=DEV)
    flat = big[4:4 + n]
    max_norm = float(inputs["max_norm"])
    for k in range(STEPS):
        g = SO.to_grid(inputs[f"g{k}"], dtype)
        gv = Views(g, lens, dtype, shift)
        for q, v in zip(params, gv.views):
            q.grad = v
        c0 = _counts()
        utils.apply_gradient(groups, state, apply_grad_to_model=apply_mode, flat_out=flat, clip_norm=max_norm)
        d = (_counts() - c0).tolist()
        assert d[0] + d[1] == codec.params_gradnorm_launches(len(lens)) and d[2] == codec.params_sgd_launches(len(lens))
        assert sum(d[3:]) == 0
        got = totals[-1]
        _check_total(got, _split(g, lens), dtype)
        c = GO.coef(got[0], max_norm, dtype)
        assert same_bits(got[1:], [c])
        assert (c < 1) == (k < 2), "the fixture's gradients: clipped in steps 0 and 1, not in step 2"
        gc = GO.clip(g, c, dtype)
        p_new, buf, d_p = SO.sgd_step(p, gc, buf, *hp, dtype=dtype)
        assert same_bits(bv.all(), bv.expect(buf)), f"buf, step {k}"
        if apply_mode:
            p = p_new
            assert same_bits(gv.all(), gv.expect(g)), "apply mode without write_clipped wrote the gradients"
            assert same_bits(host(flat), p), f"flat after step {k}"
        else:
            assert same_bits(gv.all(), gv.expect(d_p)), f"d_p after step {k}"
            assert same_bits(host(flat), d_p), f"flat after step {k}"
        assert same_bits(pv.all(), pv.expect(p)), f"params after step {k}"
        assert torch.all(big[:4] == SENTINEL) and torch.all(big[4 + n:] == SENTINEL)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_write_clipped_stores_the_clipped_gradient_between_sentinels(inputs, totals, dtype):
    from chocosgd_amd import utils
    lens = LAYOUT
    p = SO.to_grid(inputs["p0"], dtype)
    g = SO.to_grid(inputs["g0"], dtype)
    for shift in (0, 1):
        pv, gv = Views(p, lens, dtype, shift), Views(g, lens, dtype, shift)
        params = [torch.nn.Parameter(v) for v in pv.views]
        for q, v in zip(params, gv.views):
            q.grad = v
        groups = [{"params": [q], "lr": 0.1, "weight_decay": 0.0, "momentum": 0.0, "dampening": 0.0, "nesterov": False}
                  for q in params]
        utils.apply_gradient(groups, collections.defaultdict(dict), clip_norm=0.4, write_clipped=True)
        gc = GO.clip(g, GO.coef(totals[-1][0], 0.4, dtype), dtype)
        assert same_bits(gv.all(), gv.expect(gc))
        assert same_bits(pv.all(), pv.expect(SO.sgd_step(p, gc, None, 0.1, dtype=dtype)[0]))


# ----------------------------------------------------------------------------- special totals, inactive clip
def test_special_totals(inputs):
    from chocosgd_amd import utils
    hp = (0.1, 1e-4, 0.9, 0.0, False)
    lens = inputs["lens"].tolist()
    for total in (float("nan"), float("inf")):
        params, groups = _device_model(inputs["p0"], lens, hp)
        _set_grads(params, inputs["g0"], lens)
        state = collections.defaultdict(dict)
        utils.apply_gradient(groups, state, clip_norm=0.4, write_clipped=True, total_norm=total)
        got, gc = _cat(params), _cat([p.grad for p in params])
        if np.isnan(total):
            assert np.all(np.isnan(got)) and np.all(np.isnan(gc))
        else:  # c = 0: the update of a zero gradient, with the gradient's signs
            zero = GO.clip(inputs["g0"], np.float32(0))
            assert same_bits(gc, zero) and np.all(gc == 0)
            want, buf, _ = SO.sgd_step(inputs["p0"], zero, None, *hp, first=True)
            assert same_bits(got, want)
            assert same_bits(_cat([state[p]["momentum_buffer"] for p in params]), buf)


def test_inactive_clip_is_todays_apply_gradient(inputs, totals):
    """max_norm above the total: c == 1, and parameters, buffers and flat are bit-identical to
    utils.apply_gradient without clip_norm on a copy of the model."""
    from chocosgd_amd import utils
    hp = (0.1, 5e-4, 0.9, 0.0, True)
    lens = inputs["lens"].tolist()
    n = sum(lens)
    a, ga = _device_model(inputs["p0"], lens, hp)
    b, gb = _device_model(inputs["p0"], lens, hp)
    sa, sb = collections.defaultdict(dict), collections.defaultdict(dict)
    fa, fb = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    for k in range(2):
        _set_grads(a, inputs[f"g{k}"], lens)
        _set_grads(b, inputs[f"g{k}"], lens)
        utils.apply_gradient(ga, sa, flat_out=fa, clip_norm=1e6)
        utils.apply_gradient(gb, sb, flat_out=fb)
        assert totals[-1][1] == 1
        assert same_bits(_cat(a), _cat(b)) and same_bits(host(fa), host(fb))
        assert same_bits(_cat([sa[p]["momentum_buffer"] for p in a]), _cat([sb[p]["momentum_buffer"] for p in b]))
        assert same_bits(_cat([p.grad for p in a]), inputs[f"g{k}"])


# ----------------------------------------------------------------------------- master weights
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_master_steps_follow_the_fp32_trajectory(inputs, totals, dtype, shift):
    """utils.apply_gradient(master=, clip_norm=, write_clipped=True), three unpinned steps: the
    master equals the fp32 model's trajectory on the widened gradients with the fp32
    coefficient (nothing narrowed before the master lines), the parameters are its narrowing
    and p.grad receives the narrowed product.  Parameters, gradients and the fp32 momentum
    buffers are views inside one storage each (shift 0: the 16-byte path)."""
    from chocosgd_amd import codec, utils
    hp = (0.1, 1e-4, 0.9, 0.1, False)
    lens = inputs["lens"].tolist()
    p = SO.to_grid(inputs["p0"], dtype)
    pv = Views(p, lens, dtype, shift)
    params = [torch.nn.Parameter(v) for v in pv.views]
    groups = [{"params": [q], "name": f"p{i}", "lr": hp[0], "weight_decay": hp[1], "momentum": hp[2],
               "dampening": hp[3], "nesterov": hp[4]} for i, q in enumerate(params)]
    master = utils.MasterWeights(groups, [(i, gr["name"]) for i, gr in enumerate(groups)])
    buf = np.zeros(sum(lens), dtype=np.float32)
    bv = Views(buf, lens, "fp32", shift)
    state = collections.defaultdict(dict)
    for q, v in zip(params, bv.views):
        state[q]["momentum_buffer"] = v
    for k in range(STEPS):
        g = SO.to_grid(inputs[f"g{k}"], dtype)
        gv = Views(g, lens, dtype, shift)
        for q, v in zip(params, gv.views):
            q.grad = v
        c0 = _counts()
        utils.apply_gradient(groups, state, master=master, clip_norm=0.4, write_clipped=True)
        d = (_counts() - c0).tolist()
        assert d[0] + d[1] == codec.params_gradnorm_launches(len(lens))
        assert d[3] == codec.params_sgd_master_launches(len(lens)) and d[2] + sum(d[4:]) == 0
        got = totals[-1]
        _check_total(got, _split(g, lens), "fp32")
        c = GO.coef(got[0], 0.4, "fp32")
        assert same_bits(got[1:], [c])
        gc = GO.clip(g, c, "fp32")
        p, buf, _ = SO.sgd_step(p, gc, buf, *hp)
        assert same_bits(host(master.buffer), p), f"master after step {k}"
        assert same_bits(pv.all(), pv.expect(SO.to_grid(p, dtype))), "params = narrow(master)"
        assert same_bits(bv.all(), bv.expect(buf))
        assert same_bits(gv.all(), gv.expect(SO.to_grid(gc, dtype))), "p.grad = narrow(c * g)"
        if k == 0:
            assert not same_bits(SO.to_grid(gc, dtype), gc), "no product off the 16-bit grid: the case shows nothing"


# ----------------------------------------------------------------------------- the standalone drop-in
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_clip_grad_norm_matches_torch_at_the_returned_total(dtype):
    """utils.clip_grad_norm_ on 200 tensors, 171 of them with a gradient (three update chunks, two
    norm chunks): one read-and-write launch per chunk, and the gradients equal
    torch.nn.utils.clip_grads_with_norm_ on CPU copies at the total it returned."""
    from chocosgd_amd import codec, utils
    rng = np.random.RandomState(17)
    lens = rng.randint(1, 41, 200).tolist()
    lens[40], lens[90] = 9000, 0
    tdt = DTYPES[dtype]
    params = [torch.nn.Parameter(torch.zeros(m, device=DEV, dtype=tdt)) for m in lens]
    have = [i for i in range(len(lens)) if i % 7 != 3]
    gs = {i: _values([lens[i]], 100 + i, dtype) for i in have}
    for max_norm in (0.25, 1e4):
        for i in have:
            params[i].grad = dev(gs[i], tdt)
        cpu = [torch.nn.Parameter(torch.zeros(lens[i], dtype=tdt)) for i in have]
        for q, i in zip(cpu, have):
            q.grad = torch.from_numpy(gs[i].copy()).to(tdt)
        c0 = _counts()
        total = utils.clip_grad_norm_(params, max_norm)
        d = (_counts() - c0).tolist()
        assert d[0] + d[1] == codec.params_gradnorm_launches(len(have)) and d[2] == codec.params_sgd_launches(len(have))
        assert sum(d[3:]) == 0
        assert total.dim() == 0 and total.is_cuda and total.dtype == torch.float32
        _check_total(host(total).reshape(1), [gs[i] for i in have], dtype)
        torch.nn.utils.clip_grads_with_norm_(cpu, max_norm, total.cpu().to(tdt))
        assert same_bits(_cat([params[i].grad for i in have]), _cat([q.grad for q in cpu]))
        assert all(params[i].grad is None for i in range(len(lens)) if i not in have)
    pinned = utils.clip_grad_norm_(params, 0.25, total_norm=3.0)
    assert float(pinned) == 3.0


# ----------------------------------------------------------------------------- end to end
GAMMA = 0.9


def _e2e_model(dtype):
    lens = golden_json("layouts.json")["resnet20_cifar10"]
    g = torch.Generator(device=DEV).manual_seed(7)
    init = [torch.randn(m, generator=g, device=DEV).to(torch.bfloat16) for m in lens]
    params = [torch.nn.Parameter(v.to(dtype)) for v in init]
    groups = [{"params": [p], "name": f"p{i}", "lr": 0.1, "weight_decay": 0.0 if i % 3 == 1 else 5e-4, "momentum": 0.9,
               "dampening": 0.0, "nesterov": False} for i, p in enumerate(params)]
    return lens, params, groups, list(enumerate(gr["name"] for gr in groups))


def _e2e_grads(params, step, widen):
    for i, p in enumerate(params):
        gg = torch.Generator(device=DEV).manual_seed(1000 * step + i)
        g16 = torch.randn(p.shape, generator=gg, device=DEV).to(torch.bfloat16)
        p.grad = g16.float() if widen else g16.to(p.dtype)


def _choco_run(mode, pinned=None):
    """Two CHOCO steps (sign, one rank looped back on itself).  mode "fused": fused_step(state=,
    clip_norm=) on the fp32 model; "master": the same with a bf16 model and master weights;
    "split": utils.clip_grad_norm_ (pinned[k]: at that total) and then fused_step(state=) on the
    fp32 model.  Returns the per-step records."""
    from chocosgd_amd import utils
    from chocosgd_amd.parallel_choco import CHOCOCompressor
    from chocosgd_amd.tensor_buffer import TensorBuffer
    lens, params, groups, names = _e2e_model(torch.bfloat16 if mode == "master" else torch.float32)
    n = sum(lens)
    shapes = [(torch.Size([m]), m) for m in lens]
    sizes = [(m,) for m in lens]
    g = torch.Generator(device=DEV).manual_seed(8)
    hat = torch.cat([p.detach().float() for p in params]) + 0.1 * torch.randn(n, generator=g, device=DEV)
    mem = hat + 0.05 * torch.randn(n, generator=g, device=DEV)
    nhp = {0: TensorBuffer.from_flat(hat, sizes), "memory": TensorBuffer.from_flat(mem, sizes)}
    comp = CHOCOCompressor(aggregator=PS._Loopback(), comm_op="sign", comm_device="gpu", compress_ratio=0.9,
                           quantize_level=4, is_biased=False, backend="nccl", use_ipc=False)
    state = collections.defaultdict(dict)
    mw = utils.MasterWeights(groups, names) if mode == "master" else None
    out = []
    for step in range(2):
        _e2e_grads(params, step, widen=mode != "master")
        if mode == "split":
            utils.clip_grad_norm_(params, 0.4, total_norm=None if pinned is None else float(pinned[step]))
            sb = utils.fused_step(comp, groups, names, shapes, nhp, {0: 1.0}, GAMMA, 0, state=state)
        else:
            sb = utils.fused_step(comp, groups, names, shapes, nhp, {0: 1.0}, GAMMA, 0, state=state, master=mw,
                                  clip_norm=0.4)
        out.append({"x": host(mw.buffer) if mw is not None else _cat(params),
                    "msg": sb["sign_message"].contiguous().view(torch.uint8).cpu().numpy().copy(),
                    "bufs": _cat([state[p]["momentum_buffer"] for p in params]),
                    "hat": host(nhp[0].buffer), "mem": host(nhp["memory"].buffer)})
    return out


def _same_records(a, b):
    for step, (ra, rb) in enumerate(zip(a, b)):
        assert ra.keys() == rb.keys()
        for key in ra:
            if key == "msg":
                assert ra[key].size > 0 and np.array_equal(ra[key], rb[key]), (step, key)
            else:
                assert same_bits(ra[key], rb[key]), (step, key)
    assert not same_bits(a[0]["x"], a[1]["x"]), "the model did not move"


def test_fused_step_with_clip_norm_is_clip_grad_norm_then_the_step(totals):
    a = _choco_run("fused")
    assert len(totals) == 2 and all(t[1] < 1 for t in totals), "the case must clip"
    _same_records(a, _choco_run("split"))


def test_fused_step_with_master_and_clip_norm_follows_the_fp32_model(totals):
    """The bf16 model with master weights against the fp32 model on the widened gradients,
    clipped at the totals the master run measured (fp32 coefficient, nothing narrowed)."""
    a = _choco_run("master")
    pinned = [t[0] for t in totals]
    assert len(pinned) == 2 and all(t[1] < 1 for t in totals)
    _same_records(a, _choco_run("split", pinned))


class _TwoSources:
    """The exchange of a rank with one neighbour, which always sends `other`."""

    def __init__(self, other):
        self.other = other

    def _agg(self, data, op, force_wait=True):
        assert op == "get_raw_sync_data"
        return {0: data, 1: self.other}


def _dpsgd_run(mode, pinned=None):
    from chocosgd_amd import utils
    lens, params, groups, names = _e2e_model(torch.bfloat16 if mode == "master" else torch.float32)
    n = sum(lens)
    g = torch.Generator(device=DEV).manual_seed(9)
    agg = _TwoSources(torch.randn(n, generator=g, device=DEV))
    state = collections.defaultdict(dict)
    mw = utils.MasterWeights(groups, names) if mode == "master" else None
    out = []
    for step in range(2):
        _e2e_grads(params, step, widen=mode != "master")
        if mode == "split":
            utils.clip_grad_norm_(params, 0.4, total_norm=None if pinned is None else float(pinned[step]))
            bits = utils.dpsgd_step(groups, names, state, agg, {0: 0.5, 1: 0.5})
        else:
            bits = utils.dpsgd_step(groups, names, state, agg, {0: 0.5, 1: 0.5}, master=mw, clip_norm=0.4)
        assert bits == 32 * n
        out.append({"x": host(mw.buffer) if mw is not None else _cat(params),
                    "bufs": _cat([state[p]["momentum_buffer"] for p in params])})
    return out


def test_dpsgd_step_with_clip_norm_is_clip_grad_norm_then_the_step(totals):
    a = _dpsgd_run("fused")
    assert len(totals) == 2 and all(t[1] < 1 for t in totals)
    _same_records(a, _dpsgd_run("split"))


def test_dpsgd_step_with_master_and_clip_norm_follows_the_fp32_model(totals):
    a = _dpsgd_run("master")
    pinned = [t[0] for t in totals]
    assert len(pinned) == 2 and all(t[1] < 1 for t in totals)
    _same_records(a, _dpsgd_run("split", pinned))
