"""Dynamic loss scaling on the device: ParamSgdPlan.gradnorm_scaled (the unscaled total, the
coefficient over the scale, the overflow flag and the scale update in one launch), the scaled
updates (ParamSgdPlan.run / run_master(scaled=)) with their device-side skip, and the layers
above them (utils.LossScaler, apply_gradient / fused_step / dpsgd_step(loss_scale=)).

The reference has no loss scaling: everything is checked bit for bit against the numpy model
(tests/_lscale_oracle.py on _gclip_oracle and _sgd_oracle) evaluated at the device's own total,
whole storages at a time, and in fp32 against torch's own GradScaler ops.  The total alone has a
tolerance, test_gpu_gclip's: equal or adjacent on the coefficient dtype's grid to the fp64 value."""
import collections

import numpy as np
import pytest
import torch

from conftest import golden, same_bits
import _gclip_oracle as GO
import _lscale_oracle as LO
import _sgd_oracle as SO
import test_gpu_dgc_sgd as DG    # Views (tensors inside one storage between sentinels), host, dev
import test_gpu_gclip as GC      # _values, the end-to-end models and their split reference runs
import test_gpu_param_sgd as PS  # the loopback aggregator of the drop-in tests

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES, SENTINEL = DG.DTYPES, DG.SENTINEL
host, dev, Views = DG.host, DG.dev, DG.Views
_split, _cat, _values = GC._split, GC._cat, GC._values
SETS = ["clip", "wd", "mom", "nesterov", "damp"]
LAYOUT = GC.LAYOUT
SCALES = {"fp32": 1000.0, "bf16": 1000.0, "fp16": 100.0}  # not powers of two: 1 / scale is rounded
NEW = ("param_gradnorm_scaled_total_kernel", "param_sgd_scaled_kernel", "param_sgd_master_scaled_kernel")
OLD = ("param_gradnorm_total_kernel", "param_sgd_gclip_kernel", "param_sgd_master_gclip_kernel", "param_sgd_kernel",
       "param_sgd_master_kernel", "param_sqnorm_finish_kernel", "param_pack_kernel")
PASS = ("param_sqnorm_kernel",)  # the norm pass: the existing one, untouched, with and without loss scaling


@pytest.fixture(scope="module")
def inputs():
    return golden("gclip_inputs")


@pytest.fixture(scope="module")
def small():
    """140 tensors of 1-40 elements: two update chunks (72 + 68) inside one tile."""
    lens = np.random.RandomState(41).randint(1, 41, 140).tolist()
    return {"lens": lens, "p0": _values(lens, 42, "fp32"), **{f"g{k}": _values(lens, 43 + k, "fp32") for k in range(3)}}


def _counts(names):
    from chocosgd_amd import codec
    return np.array([codec.launch_count(k) for k in names])


def _scaled(g, scale, dtype):
    """The gradient a backward pass of scale * loss leaves: g times the scale, on the dtype's grid."""
    return SO.to_grid(SO.mul32(g, np.float32(scale)), dtype)


def _check_out(last, raw_split, scale, max_norm, cd):
    is_found = LO.found(raw_split)
    want = LO.total(raw_split, scale, cd)
    print("out", last, "fp64 total", want, "found", is_found)
    if np.isfinite(want):
        assert same_bits(last[:1], SO.to_grid(last[:1], cd)), "a total off its dtype's grid"
        assert GO.ulp_distance(last[0], want, cd) <= 1, (last, want)
    else:
        assert same_bits(last[:1], [want])
    assert same_bits(last, LO.out(last[0], max_norm, scale, is_found, cd)), (last, scale, is_found)
    return is_found


# ----------------------------------------------------------------------------- out[] against the model
def _gradnorm_scaled(raw, lens, dtype, max_norm, scale, shift=0, coef_dtype=None):
    from chocosgd_amd import codec, utils
    gv = Views(raw, lens, dtype, shift)
    before = gv.all()
    plan = codec.ParamSgdPlan(gv.views)
    for i, v in enumerate(gv.views):
        plan.grad_ptrs[i], plan.flags[i] = v.data_ptr(), 0
    scaler = utils.LossScaler(DEV, init_scale=scale, growth_interval=1000)
    c0 = _counts(NEW + OLD + PASS)
    a = host(plan.gradnorm_scaled(scaler, max_norm, coef_dtype=coef_dtype).clone())
    b = host(plan.gradnorm_scaled(scaler, max_norm, coef_dtype=coef_dtype).clone())
    d = (_counts(NEW + OLD + PASS) - c0).tolist()
    assert d[0] == 2 and d[0] + d[-1] == 2 * codec.params_gradnorm_launches(len(lens)) and sum(d[1:-1]) == 0, d
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "two calls, two results"
    assert same_bits(gv.all(), before), "the norm pass wrote something"
    assert scaler.get_scale() == np.float32(scale) and int(scaler._growth_tracker) == 2
    return a


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("max_norm", [None, 0.4])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_out_views_inside_one_storage(dtype, max_norm, shift):
    raw = _scaled(_values(LAYOUT, 21, dtype), SCALES[dtype], dtype)
    got = _gradnorm_scaled(raw, LAYOUT, dtype, max_norm, SCALES[dtype], shift)
    assert not _check_out(got, _split(raw, LAYOUT), np.float32(SCALES[dtype]), max_norm, dtype)
    if dtype != "fp32":  # the master path's fp32 coefficient
        got = _gradnorm_scaled(raw, LAYOUT, dtype, max_norm, SCALES[dtype], shift, coef_dtype=torch.float32)
        _check_out(got, _split(raw, LAYOUT), np.float32(SCALES[dtype]), max_norm, "fp32")


def test_out_of_more_tensors_than_the_total_launch_stages():
    """1100 tensors: the total launch reads the workspace in place; with and without an inf."""
    lens = np.random.RandomState(8).randint(1, 9, 1100).tolist()
    raw = _scaled(_values(lens, 9, "fp32"), 1000.0, "fp32")
    assert not _check_out(_gradnorm_scaled(raw, lens, "fp32", 0.25, 1000.0), _split(raw, lens), np.float32(1000.0),
                          0.25, "fp32")


def test_a_huge_finite_total_is_not_an_overflow():
    """Squares past fp32's range: the fp64 sum is finite, so found stays 0 (the fp32 total is not tested)."""
    lens = [3000, 7]
    raw = np.full(sum(lens), 1e30, dtype=np.float32)
    got = _gradnorm_scaled(raw, lens, "fp32", 0.4, 0.5)
    assert not _check_out(got, _split(raw, lens), np.float32(0.5), 0.4, "fp32")
    assert np.isfinite(got[0]) and got[0] > 1e32 and got[2] == 0 and 0 < got[1] < 1e-30


# ----------------------------------------------------------------------------- the stepping harness
class _Model:
    """Parameters, (optionally pre-existing) momentum buffers and per-step gradients as views inside
    one storage each; the numpy trajectory beside them."""

    def __init__(self, p0, lens, dtype, shift, hp, master, with_bufs=True, want_flat=True):
        from chocosgd_amd import utils
        self.lens, self.dtype, self.shift, self.hp, self.master = lens, dtype, shift, hp, master
        self.math = "fp32" if master else dtype
        self.p = SO.to_grid(p0, dtype)
        self.pv = Views(self.p, lens, dtype, shift)
        self.params = [torch.nn.Parameter(v) for v in self.pv.views]
        self.groups = [{"params": [q], "name": f"p{i}", "lr": hp[0], "weight_decay": hp[1], "momentum": hp[2],
                        "dampening": hp[3], "nesterov": bool(hp[4])} for i, q in enumerate(self.params)]
        self.mw = utils.MasterWeights(self.groups, [(i, g["name"]) for i, g in enumerate(self.groups)]) if master \
            else None
        self.state = collections.defaultdict(dict)
        self.buf = self.bv = None
        if with_bufs and hp[2] != 0:
            self.buf = np.zeros(sum(lens), dtype=np.float32)
            self.bv = Views(self.buf, lens, self.math, shift)
            for q, v in zip(self.params, self.bv.views):
                self.state[q]["momentum_buffer"] = v
        n = sum(lens)
        self.big = torch.full((n + 8,), SENTINEL, device=DEV)
        self.flat = self.big[4:4 + n] if want_flat and not master else None
        self.first = not with_bufs

    def step(self, raw, scaler, max_norm, write_clipped=True):
        """One utils.apply_gradient(loss_scale=); returns (the gradient views, out[] on the host)."""
        from chocosgd_amd import utils
        gv = Views(raw, self.lens, self.dtype, self.shift)
        for q, v in zip(self.params, gv.views):
            q.grad = v
        utils.apply_gradient(self.groups, self.state, flat_out=self.flat, master=self.mw, clip_norm=max_norm,
                             write_clipped=write_clipped, loss_scale=scaler)
        return gv, host(scaler.last.clone())

    def bufs(self):
        if self.bv is not None:
            return self.bv.all()
        return _cat([self.state[q]["momentum_buffer"] for q in self.params])

    def check(self, gv, raw, last, taken, write_clipped=True, what=""):
        """Advance the numpy trajectory (taken) and compare every storage with it."""
        want_g = raw
        if taken:
            gu = LO.unscale(raw, last[1], self.math)
            self.p, buf, _ = SO.sgd_step(self.p if not self.master else self.m(), gu, self.buf, *self.hp,
                                         first=self.first, dtype=self.math)
            if self.master:
                self._m = self.p
            if buf is not None:
                self.buf, self.first = buf, False
            if write_clipped:
                want_g = SO.to_grid(gu, self.dtype)
        assert same_bits(gv.all(), gv.expect(want_g)), f"gradients {what}"
        if self.master:
            assert same_bits(host(self.mw.buffer), self.m()), f"master {what}"
            assert same_bits(self.pv.all(), self.pv.expect(SO.to_grid(self.m(), self.dtype))), f"params {what}"
        else:
            assert same_bits(self.pv.all(), self.pv.expect(self.p)), f"params {what}"
            if self.flat is not None:
                assert same_bits(host(self.flat), self.p), f"flat {what}"
        if self.hp[2] != 0 and not self.first:
            got = self.bufs()
            assert same_bits(got, self.bv.expect(self.buf) if self.bv is not None else self.buf), f"buffers {what}"
        assert torch.all(self.big[:4] == SENTINEL) and torch.all(self.big[-4:] == SENTINEL)

    def m(self):
        """The master's numpy trajectory (starts as the widened parameters)."""
        if not hasattr(self, "_m"):
            self._m = self.p.copy()
        return self._m


def _hp(name):
    lr, wd, mom, damp, nest = golden(f"gclip_{name}")["hp"].tolist()
    return lr, wd, mom, damp, bool(nest)


# ----------------------------------------------------------------------------- taken steps
@pytest.mark.parametrize("master", [False, True], ids=["plain", "master"])
@pytest.mark.parametrize("name", SETS)
def test_taken_steps_match_the_model_at_the_device_total(inputs, name, master):
    """Three steps per hyperparameter set, fp16 at shift 0 and bf16 at shift 1, max_norm 0.4."""
    from chocosgd_amd import utils
    for dtype, shift in (("fp16", 0), ("bf16", 1)):
        mdl = _Model(inputs["p0"], LAYOUT, dtype, shift, _hp(name), master)
        scaler = utils.LossScaler(DEV, init_scale=SCALES[dtype], growth_interval=1000)
        for k in range(3):
            raw = _scaled(SO.to_grid(inputs[f"g{k}"], dtype), SCALES[dtype], dtype)
            gv, last = mdl.step(raw, scaler, 0.4)
            assert not _check_out(last, _split(raw, LAYOUT), np.float32(SCALES[dtype]), 0.4, mdl.math if master else dtype)
            mdl.check(gv, raw, last, True, what=f"{dtype} step {k}")
        assert not scaler.skipped() and int(scaler._growth_tracker) == 3


@pytest.mark.parametrize("master", [False, True], ids=["plain", "master"])
def test_taken_steps_fp32_and_no_clip_and_no_write_clipped(inputs, master):
    from chocosgd_amd import utils
    mdl = _Model(inputs["p0"], LAYOUT, "fp32", 0, _hp("damp"), master)
    scaler = utils.LossScaler(DEV, init_scale=1000.0)
    for k in range(2):
        raw = _scaled(inputs[f"g{k}"], 1000.0, "fp32")
        gv, last = mdl.step(raw, scaler, None, write_clipped=k == 1)
        assert not _check_out(last, _split(raw, LAYOUT), np.float32(1000.0), None, "fp32")
        mdl.check(gv, raw, last, True, write_clipped=k == 1, what=f"step {k}")


# ----------------------------------------------------------------------------- skipped steps
PLACES = {"one element": ("layout", 1, 0, np.inf), "tile crossing": ("layout", 3, 8187, np.nan),
          "last of chunk 2": ("small", 139, -1, -np.inf)}


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("master", [False, True], ids=["plain", "master"])
@pytest.mark.parametrize("place", sorted(PLACES))
def test_a_skipped_step_changes_nothing_and_backs_off(inputs, small, place, master, shift):
    """Taken, skipped (one non-finite element), taken: the skipped step leaves every storage
    bit-identical, flat = the pack of the unchanged parameters, scale halved, tracker 0."""
    from chocosgd_amd import utils
    which, tensor, elem, value = PLACES[place]
    src, lens = (inputs, LAYOUT) if which == "layout" else (small, small["lens"])
    dtype = "fp16"
    mdl = _Model(src["p0"], lens, dtype, shift, (0.1, 1e-4, 0.9, 0.1, False), master)
    scaler = utils.LossScaler(DEV, init_scale=64.0, growth_interval=1000)
    scale = np.float32(64.0)
    for k in range(3):
        raw = _scaled(SO.to_grid(src[f"g{k}"], dtype), scale, dtype)
        if k == 1:
            raw[int(np.sum(lens[:tensor])) + (elem if elem >= 0 else lens[tensor] - 1)] = value
            if mdl.flat is not None:
                mdl.flat.fill_(SENTINEL)
        gv, last = mdl.step(raw, scaler, 0.4)
        is_found = _check_out(last, _split(raw, lens), scale, 0.4, mdl.math if master else dtype)
        assert is_found == (k == 1) == scaler.skipped()
        mdl.check(gv, raw, last, not is_found, what=f"step {k}")
        scale = np.float32(32.0) if k >= 1 else scale
        assert scaler.get_scale() == scale and int(scaler._growth_tracker) == (1, 0, 1)[k]


@pytest.mark.parametrize("master", [False, True], ids=["plain", "master"])
def test_a_skipped_first_step_leaves_no_buffers(inputs, master):
    """dampening != 0 and no momentum buffer yet: an overflowed first step is rolled back on the
    host (no buffer left, flat = the pack of the unchanged parameters), and the next step runs the
    FIRST lines."""
    from chocosgd_amd import utils
    dtype = "fp16"
    mdl = _Model(inputs["p0"], LAYOUT, dtype, 0, (0.1, 1e-4, 0.9, 0.1, False), master, with_bufs=False)
    scaler = utils.LossScaler(DEV, init_scale=64.0)
    raw = _scaled(SO.to_grid(inputs["g0"], dtype), 64.0, dtype)
    raw[7] = np.inf
    gv, last = mdl.step(raw, scaler, 0.4)
    assert _check_out(last, _split(raw, LAYOUT), np.float32(64.0), 0.4, mdl.math if master else dtype)
    mdl.check(gv, raw, last, False, what="skipped first step")
    assert all("momentum_buffer" not in mdl.state[q] for q in mdl.params) and scaler.get_scale() == 32.0
    for k in (1, 2):
        raw = _scaled(SO.to_grid(inputs[f"g{k}"], dtype), 32.0, dtype)
        gv, last = mdl.step(raw, scaler, 0.4)
        assert not _check_out(last, _split(raw, LAYOUT), np.float32(32.0), 0.4, mdl.math if master else dtype)
        mdl.check(gv, raw, last, True, what=f"step {k}")


# ----------------------------------------------------------------------------- growth
def test_the_scale_doubles_after_two_taken_steps_and_the_next_step_uses_it(inputs):
    from chocosgd_amd import utils
    mdl = _Model(inputs["p0"], LAYOUT, "fp16", 0, (0.1, 0.0, 0.9, 0.0, False), True)
    scaler = utils.LossScaler(DEV, init_scale=24.0, growth_interval=2)
    scale, tracker = np.float32(24.0), 0
    for k in range(3):
        raw = _scaled(SO.to_grid(inputs[f"g{k}"], "fp16"), scale, "fp16")
        gv, last = mdl.step(raw, scaler, None)
        assert not _check_out(last, _split(raw, LAYOUT), scale, None, "fp32") and last[3] == scale
        mdl.check(gv, raw, last, True, what=f"step {k}")
        scale, tracker = LO.update(scale, tracker, False, interval=2)
        assert scaler.get_scale() == scale and int(scaler._growth_tracker) == tracker
    assert scale == 48.0


# ----------------------------------------------------------------------------- fp32 against torch's GradScaler ops
def test_fp32_step_equals_torchs_unscale_clip_and_update_on_the_device(inputs):
    """A power-of-two scale: multiplying by 1 / scale is exact, so the scaled step equals
    _amp_foreach_non_finite_check_and_unscale_, clip_grad_norm_loop at the same total,
    apply_gradient_loop and _amp_update_scale_ on a twin model, bit for bit."""
    from chocosgd_amd import utils
    hp = (0.1, 5e-4, 0.9, 0.0, True)
    lens = inputs["lens"].tolist()
    a, ga = GC._device_model(inputs["p0"], lens, hp)
    b, gb = GC._device_model(inputs["p0"], lens, hp)
    sa, sb = collections.defaultdict(dict), collections.defaultdict(dict)
    scaler = utils.LossScaler(DEV, init_scale=4096.0, growth_interval=2)
    scale_b, tracker_b = torch.full((1,), 4096.0, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    for k in range(3):
        raw = SO.mul32(inputs[f"g{k}"], host(scale_b)[0])
        GC._set_grads(a, raw, lens)
        GC._set_grads(b, raw, lens)
        utils.apply_gradient(ga, sa, clip_norm=0.4, write_clipped=True, loss_scale=scaler)
        found = torch.zeros(1, device=DEV)
        torch._amp_foreach_non_finite_check_and_unscale_([q.grad for q in b], found, scale_b.double().reciprocal().float())
        utils.clip_grad_norm_loop(b, 0.4, total_norm=scaler.last[0])
        utils.apply_gradient_loop(gb, sb)
        torch._amp_update_scale_(scale_b, tracker_b, found, 2.0, 0.5, 2)
        assert same_bits(_cat(a), _cat(b)), f"params after step {k}"
        assert same_bits(_cat([q.grad for q in a]), _cat([q.grad for q in b])), f"gradients after step {k}"
        assert same_bits(_cat([sa[q]["momentum_buffer"] for q in a]), _cat([sb[q]["momentum_buffer"] for q in b]))
        assert torch.equal(scaler._scale, scale_b) and torch.equal(scaler._growth_tracker, tracker_b)
    assert scaler.get_scale() == 8192.0


# ----------------------------------------------------------------------------- launches and syncs
@pytest.mark.parametrize("master", [False, True], ids=["plain", "master"])
def test_launch_counts(inputs, master):
    """A scaled step, clipped or not, takes exactly the launches of today's clipped step, under the
    new site names (the norm pass is the existing one); neither path hits the other's sites."""
    from chocosgd_amd import codec, utils
    names = NEW + OLD + PASS
    hp = (0.1, 1e-4, 0.9, 0.0, False)
    scaler = utils.LossScaler(DEV, init_scale=64.0)
    raw = _scaled(SO.to_grid(inputs["g0"], "fp16"), 64.0, "fp16")

    def run(**kw):
        mdl = _Model(inputs["p0"], LAYOUT, "fp16", 0, hp, master)
        gv = Views(raw, LAYOUT, "fp16", 0)
        for q, v in zip(mdl.params, gv.views):
            q.grad = v
        c0 = _counts(names)
        utils.apply_gradient(mdl.groups, mdl.state, flat_out=mdl.flat, master=mdl.mw, **kw)
        return dict(zip(names, (_counts(names) - c0).tolist()))

    today = run(clip_norm=0.4)
    upd_old = "param_sgd_master_gclip_kernel" if master else "param_sgd_gclip_kernel"
    upd_new = "param_sgd_master_scaled_kernel" if master else "param_sgd_scaled_kernel"
    assert all(today[k] == 0 for k in NEW) and today[upd_old] == codec.params_sgd_launches(len(LAYOUT))
    assert today["param_gradnorm_total_kernel"] == 1
    for kw in (dict(clip_norm=0.4), dict()):
        d = run(loss_scale=scaler, **kw)
        assert all(d[k] == 0 for k in OLD), d
        assert d["param_gradnorm_scaled_total_kernel"] == 1 and d[upd_new] == today[upd_old]
        assert d["param_sqnorm_kernel"] == today["param_sqnorm_kernel"] and sum(d.values()) == sum(today.values())
    plain = run()
    assert all(plain[k] == 0 for k in NEW)


def test_no_host_sync_in_steady_state(inputs):
    """After the first taken step (which creates the buffers and reads `found`), a step syncs nothing."""
    from chocosgd_amd import utils
    mdl = _Model(inputs["p0"], LAYOUT, "fp16", 0, (0.1, 1e-4, 0.9, 0.1, False), True, with_bufs=False)
    scaler = utils.LossScaler(DEV, init_scale=64.0)
    raws = [_scaled(SO.to_grid(inputs[f"g{k}"], "fp16"), 64.0, "fp16") for k in range(2)]
    raws[1][100] = np.inf  # the steady-state step is a skipped one: the skip is the device's
    gv, last = mdl.step(raws[0], scaler, 0.4)
    mdl.check(gv, raws[0], last, True, what="first step")
    gv = Views(raws[1], LAYOUT, "fp16", 0)
    for q, v in zip(mdl.params, gv.views):
        q.grad = v
    probe = torch.ones(1, device=DEV)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            armed = False
        except RuntimeError:
            armed = True
        if armed:
            utils.apply_gradient(mdl.groups, mdl.state, master=mdl.mw, clip_norm=0.4, write_clipped=True,
                                 loss_scale=scaler)
            loss = scaler.scale(probe)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    if not armed:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not catch .item() on this build")
    assert scaler.skipped() and float(loss) == 32.0
    mdl.check(gv, raws[1], host(scaler.last), False, what="skipped step")


# ----------------------------------------------------------------------------- end to end
def _choco_scaled(bad_step=None):
    """GC._choco_run("master") with the gradients multiplied by 1024 and loss_scale=: a bf16 model
    with master weights, clip_norm 0.4.  bad_step: that step's first gradient holds an inf."""
    from chocosgd_amd import utils
    from chocosgd_amd.parallel_choco import CHOCOCompressor
    from chocosgd_amd.tensor_buffer import TensorBuffer
    lens, params, groups, names = GC._e2e_model(torch.bfloat16)
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
    mw = utils.MasterWeights(groups, names)
    scaler = utils.LossScaler(DEV, init_scale=1024.0)
    out = []
    for step in range(2):
        GC._e2e_grads(params, step, widen=False)
        for p in params:
            p.grad.mul_(1024.0)  # exact in bf16
        if step == bad_step:
            params[0].grad[0] = float("inf")
        sb = utils.fused_step(comp, groups, names, shapes, nhp, {0: 1.0}, GC.GAMMA, 0, state=state, master=mw,
                              clip_norm=0.4, loss_scale=scaler)
        out.append({"x": host(mw.buffer), "msg": sb["sign_message"].contiguous().view(torch.uint8).cpu().numpy().copy(),
                    "bufs": _cat([state[p]["momentum_buffer"] for p in params]),
                    "hat": host(nhp[0].buffer), "mem": host(nhp["memory"].buffer),
                    "params": _cat(params), "skipped": scaler.skipped(), "scale": scaler.get_scale()})
    return out


def test_fused_step_with_loss_scale_follows_the_unscaled_master_run():
    """A power-of-two scale is exact: the scaled run equals today's fused_step(master=, clip_norm=)
    on the unscaled gradients, record for record."""
    a = _choco_scaled()
    assert [r["skipped"] for r in a] == [False, False]
    keys = ("x", "msg", "bufs", "hat", "mem")
    GC._same_records([{k: r[k] for k in keys} for r in a], GC._choco_run("master"))


def test_fused_step_skipped_step_leaves_the_update_out_and_still_gossips():
    a, b = _choco_scaled(bad_step=1), _choco_scaled()
    assert [r["skipped"] for r in a] == [False, True] and [r["scale"] for r in a] == [1024.0, 512.0]
    for key in ("x", "msg", "bufs", "hat", "mem"):
        assert np.array_equal(a[0][key], b[0][key])
    assert same_bits(a[1]["bufs"], a[0]["bufs"]), "a skipped step wrote the momentum buffers"
    assert a[1]["msg"].size > 0 and not same_bits(a[1]["hat"], a[0]["hat"]), "the skipped step did not gossip"
    assert not same_bits(a[1]["x"], a[0]["x"]) and not same_bits(a[1]["x"], b[1]["x"])
    assert same_bits(a[1]["params"], SO.to_grid(a[1]["x"], "bf16")), "params = narrow(x) after the unpack"


def test_dpsgd_step_with_loss_scale_taken_and_skipped():
    """Step 0 equals today's dpsgd_step(master=, clip_norm=) on the unscaled gradients; the
    skipped step 1 mixes the unchanged x with the neighbour's (the reference's own expression)."""
    from chocosgd_amd import utils
    lens, params, groups, names = GC._e2e_model(torch.bfloat16)
    n = sum(lens)
    g = torch.Generator(device=DEV).manual_seed(9)
    other = torch.randn(n, generator=g, device=DEV)
    agg = GC._TwoSources(other)
    state = collections.defaultdict(dict)
    mw = utils.MasterWeights(groups, names)
    scaler = utils.LossScaler(DEV, init_scale=1024.0)
    want = GC._dpsgd_run("master")
    for step in range(2):
        GC._e2e_grads(params, step, widen=False)
        for p in params:
            p.grad.mul_(1024.0)
        if step == 1:
            params[3].grad[-1] = float("nan")
        x0, b0 = mw.buffer.clone(), _cat([state[p]["momentum_buffer"] for p in params]) if step else None
        bits = utils.dpsgd_step(groups, names, state, agg, {0: 0.5, 1: 0.5}, master=mw, clip_norm=0.4, loss_scale=scaler)
        assert bits == 32 * n and scaler.skipped() == (step == 1)
        if step == 0:
            assert same_bits(host(mw.buffer), want[0]["x"])
            assert same_bits(_cat([state[p]["momentum_buffer"] for p in params]), want[0]["bufs"])
        else:
            assert torch.equal(mw.buffer, utils.weighted_sum([x0, other], [0.5, 0.5])), "the mix of the unchanged x"
            assert same_bits(_cat([state[p]["momentum_buffer"] for p in params]), b0)
            assert same_bits(_cat(params), SO.to_grid(host(mw.buffer), "bf16")) and scaler.get_scale() == 512.0
