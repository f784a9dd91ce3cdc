"""The batched SGD update fused with the pack, on the device: codec.params_sgd (csrc/sgd.hip)
and the layers above it (utils.apply_gradient, utils.fused_step(state=...)).

Everything is compared bit for bit: the fp32 fixtures are the reference's own results
(tests/golden/sgd_*.npz), every other case is checked against the numpy restatement of the
documented per-element model (tests/_sgd_oracle.py), whole storages at a time, so that every
byte a launch does not own is checked together with the ones it does."""
import collections

import numpy as np
import pytest
import torch

from conftest import golden, golden_json, same_bits
import _sgd_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda"
GAMMA = 0.9
CAP = 72  # tensors per launch (sgd.hip kSgdCap)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
NAMES = {v: k for k, v in DTYPES.items()}
SENTINEL = -7.0  # exact in every dtype
SETS = ["plain", "wd", "mom", "nesterov", "damp"]
STEPS = 3


def host(t):
    return t.detach().float().cpu().numpy()


def _counts():
    from chocosgd_amd import codec
    return codec.launch_count("param_sgd_kernel"), codec.launch_count("param_pack_kernel")


# ----------------------------------------------------------------------------- fixture replay
def _device_model(inputs, hp):
    lr, wd, mom, damp, nest = hp
    lens = inputs["lens"].tolist()
    params, o = [], 0
    for m in lens:
        params.append(torch.nn.Parameter(torch.from_numpy(inputs["p0"][o:o + m].copy()).to(DEV)))
        o += m
    groups = [{"params": [p], "lr": lr, "weight_decay": wd, "momentum": mom, "dampening": damp, "nesterov": bool(nest)}
              for p in params]
    return params, groups, lens


def _cat(tensors):
    return np.concatenate([host(t).reshape(-1) for t in tensors])


@pytest.mark.parametrize("with_flat", [True, False])
@pytest.mark.parametrize("mode", ["apply", "grad"])
@pytest.mark.parametrize("name", SETS)
def test_fixture_replay(name, mode, with_flat):
    """The reference's three steps replayed through utils.apply_gradient on the device: p, buf,
    the grads and flat after every step, and the launches the steps took."""
    from chocosgd_amd import codec, utils
    inputs, fx = golden("sgd_inputs"), golden(f"sgd_{name}_{mode}")
    hp = fx["hp"].tolist()
    params, groups, lens = _device_model(inputs, hp)
    n = sum(lens)
    state = collections.defaultdict(dict)
    big = torch.full((n + 8,), SENTINEL, device=DEV)
    flat = big[4:4 + n] if with_flat else None
    s0, k0 = _counts()
    for k in range(STEPS):
        o = 0
        for p, m in zip(params, lens):
            p.grad = torch.from_numpy(inputs[f"g{k}"][o:o + m].copy()).to(DEV)
            o += m
        grads = [p.grad for p in params]
        utils.apply_gradient(groups, state, apply_grad_to_model=mode == "apply", flat_out=flat)
        assert same_bits(_cat(params), fx[f"p{k}"]), f"p after step {k}"
        if hp[2] != 0:
            assert same_bits(_cat([state[p]["momentum_buffer"] for p in params]), fx[f"buf{k}"]), f"buf, step {k}"
        assert all(p.grad is g for p, g in zip(params, grads))
        if mode == "grad":
            assert same_bits(_cat(grads), fx[f"d{k}"]), f"d_p after step {k}"
        else:
            assert same_bits(_cat(grads), inputs[f"g{k}"]), "apply mode wrote the grads"
        if with_flat:
            assert same_bits(host(flat), fx[f"d{k}" if mode == "grad" else f"p{k}"]), f"flat after step {k}"
            assert torch.all(big[:4] == SENTINEL) and torch.all(big[4 + n:] == SENTINEL)
    s1, k1 = _counts()
    assert s1 - s0 == STEPS * codec.params_sgd_launches(len(lens)) and k1 == k0


# ----------------------------------------------------------------------------- layouts
SPECIAL = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-41, -1e-41, 6e-8, 65519.0, -70000.0, 3e38, 1e-30]


def _values(m, seed, lo, hi):
    """Values over several decades with the special ones sprinkled in (where there is room)."""
    rng = np.random.RandomState(seed)
    v = (rng.standard_normal(m) * 10.0 ** rng.uniform(lo, hi, m)).astype(np.float32)
    if m >= 64:
        pos = rng.choice(m, len(SPECIAL), replace=False)
        v[pos] = np.array(SPECIAL, dtype=np.float32)[rng.permutation(len(SPECIAL))]
    return v


class Guarded:
    """Tensors as views into ONE storage per dtype: `lead` sentinel elements, then each tensor
    followed by `gap` sentinels.  Separate allocations (own=True) give every tensor its own."""

    def __init__(self, lens, dtypes, seed, lo, hi, lead=0, gap=8, own=False):
        self.stores, self.where, self.views = [], [], []
        by_dtype = {}
        for i, (m, dt) in enumerate(zip(lens, dtypes)):
            key = (dt, i) if own else dt
            by_dtype.setdefault(key, []).append(i)
        slot = {}
        for key, idx in by_dtype.items():
            dt = key[0] if own else key
            total = lead + sum(lens[i] + gap for i in idx)
            store = torch.full((total,), SENTINEL, device=DEV, dtype=dt)
            p = lead
            for i in idx:
                store[p:p + lens[i]] = torch.from_numpy(_values(lens[i], seed + i, lo, hi)).to(DEV).to(dt)
                slot[i] = (len(self.stores), p)
                p += lens[i] + gap
            self.stores.append(store)
        for i, m in enumerate(lens):
            s, p = slot[i]
            self.where.append((s, p, m))
            self.views.append(self.stores[s][p:p + m])
        self.before = [s.clone() for s in self.stores]

    def expected(self, new_values):
        """The storages with tensor i's elements replaced by new_values[i] (None: unchanged)."""
        want = [s.clone() for s in self.before]
        for (s, p, m), v in zip(self.where, new_values):
            if v is not None:
                want[s][p:p + m] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(DEV).to(want[s].dtype)
        return want

    def check(self, new_values, what):
        for got, want in zip(self.stores, self.expected(new_values)):
            assert same_bits(host(got), host(want)), what


def _varied_hp(i):
    """lr, wd, mom, damp, nesterov differing inside one launch: wd 0 on every other tensor (the
    batch-norm case), one tensor in seven without momentum, Nesterov and dampening mixed in."""
    wd = 0.0 if i % 2 else 5e-4
    mom = 0.0 if i % 7 == 3 else 0.9
    nest = mom != 0 and i % 3 == 0
    damp = 0.1 if (mom != 0 and not nest and i % 4 == 1) else 0.0
    return 0.1 / (1 + i % 5), wd, mom, damp, nest


def _dtypes(mode, k):
    return [DTYPES[mode] if mode != "mixed" else list(DTYPES.values())[i % 3] for i in range(k)]


def run_case(lens, mode, lead=(0, 0, 0), gap=8, own=False, flat_shift=4, nograd=(), hp=_varied_hp, first=lambda i: i % 2 == 0,
             grad_mode=False, write=True, seed=1000):
    """One codec.params_sgd call on guarded storages against the oracle; returns the launches."""
    from chocosgd_amd import codec
    k, n = len(lens), sum(lens)
    dts = _dtypes(mode, k)
    P = Guarded(lens, dts, seed, -3, 1, lead[0], gap, own)
    G = Guarded(lens, dts, seed + 5000, -4, 0, lead[1], gap, own)
    B = Guarded(lens, dts, seed + 9000, -4, 0, lead[2], gap, own)
    hps = [hp(i) for i in range(k)]
    firsts = [bool(first(i)) and hps[i][2] != 0 for i in range(k)]
    big = flat = None
    if flat_shift is not None:
        big = torch.full((n + 2 * flat_shift + 8,), SENTINEL, device=DEV)
        flat = big[flat_shift:flat_shift + n]
    new_p, new_g, new_b, new_flat = [], [], [], []
    for i in range(k):
        pw, gw, bw = host(P.views[i]), host(G.views[i]), host(B.views[i])
        if i in nograd:
            new_p.append(None), new_g.append(None), new_b.append(None), new_flat.append(pw)
            continue
        lr, wd, mom, damp, nest = hps[i]
        p_new, b_new, d = SO.sgd_step(pw, gw, bw, lr, wd, mom, damp, nest, firsts[i], dtype=NAMES[dts[i]])
        new_p.append(p_new if (write and not grad_mode) else None)
        new_g.append(d if (write and grad_mode) else None)
        new_b.append(b_new)
        new_flat.append(d if grad_mode else p_new)
    s0, k0 = _counts()
    codec.params_sgd(P.views, [None if i in nograd else g for i, g in enumerate(G.views)],
                     [b if hps[i][2] != 0 else None for i, b in enumerate(B.views)],
                     [h[0] for h in hps], [h[1] for h in hps], [h[2] for h in hps], [h[3] for h in hps],
                     [h[4] for h in hps], firsts, flat=flat, grad_mode=grad_mode, write=write)
    s1, k1 = _counts()
    P.check(new_p, "params (or their guards)")
    G.check(new_g, "grads (or their guards)")
    B.check(new_b, "momentum buffers (or their guards)")
    if flat is not None:
        want = torch.full_like(big, SENTINEL)
        if n:
            want[flat_shift:flat_shift + n] = torch.from_numpy(np.concatenate(new_flat).astype(np.float32)).to(DEV)
        assert same_bits(host(big), host(want)), "flat (or its guards)"
    assert k1 == k0, "a pack launch was made"
    assert s1 - s0 == codec.params_sgd_launches(k)
    return s1 - s0


MODES = ["fp32", "bf16", "fp16", "mixed"]
BASE = [1, 2, 3, 7, 8, 9, 31, 33, 4097, 16, 8200, 20]


@pytest.mark.parametrize("gap", [1, 2, 3])
@pytest.mark.parametrize("mode", MODES)
def test_views_at_element_alignment(mode, gap):
    """Views into one allocation whose element offsets run through every residue modulo 4
    (lead 1, gaps 1 / 2 / 3): the elementwise path, and nothing next to a tensor is touched."""
    run_case(BASE, mode, lead=(1, 1, 1), gap=gap)
    run_case(BASE, mode, lead=(1, 1, 1), gap=gap, grad_mode=True)


@pytest.mark.parametrize("off", ["g", "buf", "p"])
@pytest.mark.parametrize("mode", MODES)
def test_mixed_congruence_falls_back(mode, off):
    """Two sides 16-byte aligned and one an element off (each tensor its own allocation, so a
    vector access of the misaligned side would show in its guards or values)."""
    lead = {"p": (1, 0, 0), "g": (0, 1, 0), "buf": (0, 0, 1)}[off]
    run_case([40, 8192 + 24, 7, 300], mode, lead=lead, own=True, first=lambda i: False)


@pytest.mark.parametrize("mode", MODES)
def test_a_tensor_across_several_tiles(mode):
    """Ends inside tiles, whole tiles between; the vector path with cut groups at both ends."""
    run_case([100, 3 * 8192 + 77, 50], mode, gap=8)
    run_case([5, 2 * 8192 + 3, 8192, 11], mode, gap=8, own=True, grad_mode=True)


@pytest.mark.parametrize("count", [CAP - 1, CAP, CAP + 1, 2 * CAP + 3])
def test_chunk_boundaries_inside_a_tile(count):
    lens = [1 + i % 13 for i in range(count)]
    assert run_case(lens, "mixed", gap=8) == -(-count // CAP)
    assert run_case(lens, "fp32", gap=1, lead=(1, 1, 1)) == -(-count // CAP)


@pytest.mark.parametrize("mode", MODES)
def test_zero_length_and_no_grad_tensors(mode):
    run_case([0, 5, 0, 0, 4100, 0], mode)
    # a tensor without a gradient between two updated ones: packed, nothing else written
    run_case([300, 8195, 40, 9000, 7], mode, nograd=(1, 2))
    run_case([300, 8195, 40], mode, nograd=(1,), write=False)


@pytest.mark.parametrize("mode", MODES)
def test_flat_alignment_and_no_flat(mode):
    run_case(BASE, mode, flat_shift=1)                    # flat at 4-byte alignment: elementwise
    run_case(BASE, mode, flat_shift=None)                 # no flat side: params only
    run_case(BASE, mode, flat_shift=None, grad_mode=True)
    run_case([8192 * 2 + 8], mode, flat_shift=None, own=True)


@pytest.mark.parametrize("mode", MODES)
def test_write_off_leaves_params_and_grads_alone(mode):
    """run_case compares whole storages: with write off the params (apply mode) and the grads
    (grad mode) must come back bit-identical, in apply mode the grads always do."""
    run_case(BASE, mode, write=False)
    run_case(BASE, mode, write=False, grad_mode=True)
    run_case([8192 + 16, 64], mode, write=False, own=True)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_uniform_hyperparameter_sets(mode):
    """Each of the fixture's five sets on one layout, steady state and first step."""
    for lr, wd, mom, damp, nest in [(0.1, 0, 0, 0, False), (0.05, 1e-4, 0, 0, False), (0.1, 0, 0.9, 0, False),
                                    (0.1, 5e-4, 0.9, 0, True), (0.01, 1e-4, 0.9, 0.1, False)]:
        for fst in (True, False):
            run_case([33, 8195, 4099], mode, hp=lambda i: (lr, wd, mom, damp, nest), first=lambda i: fst)


def test_grad_and_buffer_in_the_same_memory():
    """g and buf of a tensor may be one tensor (after the reference's grad mode p.grad IS the
    buffer): every element reads both before it writes."""
    from chocosgd_amd import codec
    for dt in DTYPES.values():
        m = 8192 + 40
        p = torch.from_numpy(_values(m, 1, -3, 1)).to(DEV).to(dt)
        gb = torch.from_numpy(_values(m, 2, -4, 0)).to(DEV).to(dt)
        pw, gw = host(p), host(gb)
        p_new, b_new, d = SO.sgd_step(pw, gw, gw, 0.1, 1e-4, 0.9, 0.0, False, False, dtype=NAMES[dt])
        flat = torch.empty(m, device=DEV)
        codec.params_sgd([p], [gb], [gb], 0.1, 1e-4, 0.9, flat=flat)
        assert same_bits(host(p), p_new) and same_bits(host(gb), b_new) and same_bits(host(flat), p_new)


def test_python_entry_points_refuse_what_the_kernel_cannot_take():
    from chocosgd_amd import codec
    p, g = torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)
    with pytest.raises(RuntimeError):  # a gradient of another dtype
        codec.params_sgd([p], [g.half()], [None], 0.1)
    with pytest.raises(RuntimeError):  # flat of the wrong length
        codec.params_sgd([p], [g], [None], 0.1, flat=torch.zeros(9, device=DEV))
    with pytest.raises(RuntimeError, match="nesterov"):
        codec.params_sgd([p], [g], [None], 0.1, nesterov=True)
    with pytest.raises(RuntimeError):  # CPU tensors
        codec.params_sgd([p.cpu()], [g.cpu()], [None], 0.1)


def test_apply_gradient_falls_back_to_the_loop_with_the_same_bits():
    """A non-contiguous gradient: the per-tensor loop runs (no launch of the kernel), a first-step
    buffer is still built by the first-step rule, and fp32 results are the kernel's."""
    from chocosgd_amd import utils
    p0, g0 = _values(600, 3, -3, 1), _values(600, 4, -4, 0)
    want = SO.sgd_step(p0, g0, None, 0.1, 1e-4, 0.9, 0.1, False, True)
    for contiguous in (True, False):
        p = torch.nn.Parameter(torch.from_numpy(p0).to(DEV).view(20, 30))
        g = torch.from_numpy(g0).to(DEV).view(20, 30)
        p.grad = g if contiguous else g.t().contiguous().t()  # the same values, other strides
        assert p.grad.is_contiguous() == contiguous
        groups = [{"params": [p], "lr": 0.1, "weight_decay": 1e-4, "momentum": 0.9, "dampening": 0.1,
                   "nesterov": False}]
        state = collections.defaultdict(dict)
        s0, _ = _counts()
        flat = torch.empty(600, device=DEV)
        utils.apply_gradient(groups, state, flat_out=flat)
        assert (_counts()[0] - s0) == (1 if contiguous else 0)
        assert same_bits(host(p).reshape(-1), want[0]) and same_bits(host(flat), want[0])
        assert same_bits(host(state[p]["momentum_buffer"]).reshape(-1), want[1])
        assert same_bits(host(p.grad).reshape(-1), g0), "apply mode wrote the grad"


# ----------------------------------------------------------------------------- the drop-in
class _Loopback:
    def _agg(self, data, op, force_wait=False):
        return [], {0: data}

    def complete_wait(self, reqs):
        pass


_MESSAGE = {"compress_top_k": lambda sb: sb["wire_message"], "sign": lambda sb: sb["sign_message"]}


def _dropin_run(op, dtype, defer, fused):
    from chocosgd_amd import utils
    from chocosgd_amd.parallel_choco import CHOCOCompressor
    from chocosgd_amd.tensor_buffer import TensorBuffer
    lens = golden_json("layouts.json")["resnet20_cifar10"]
    n = sum(lens)
    g = torch.Generator(device=DEV).manual_seed(7)
    params = [torch.nn.Parameter(torch.randn(m, generator=g, device=DEV).to(dtype)) for m in lens]
    groups = [{"params": [p], "name": f"p{i}", "lr": 0.1, "weight_decay": 0.0 if i % 3 == 1 else 5e-4, "momentum": 0.9,
               "dampening": 0.0, "nesterov": False} for i, p in enumerate(params)]
    names = list(enumerate(gr["name"] for gr in groups))
    shapes = [(torch.Size([m]), m) for m in lens]
    sizes = [(m,) for m in lens]
    hat = torch.cat([p.detach().float() for p in params]) + 0.1 * torch.randn(n, generator=g, device=DEV)
    mem = hat + 0.05 * torch.randn(n, generator=g, device=DEV)
    nhp = {0: TensorBuffer.from_flat(hat, sizes), "memory": TensorBuffer.from_flat(mem, sizes)}
    comp = CHOCOCompressor(aggregator=_Loopback(), comm_op=op, comm_device="gpu", compress_ratio=0.9,
                           quantize_level=4, is_biased=False, backend="nccl", use_ipc=False)
    state = collections.defaultdict(dict)
    torch.manual_seed(1234)
    out = []
    for step in range(STEPS):
        for i, p in enumerate(params):
            gg = torch.Generator(device=DEV).manual_seed(1000 * step + i)
            p.grad = (0.1 * torch.randn(p.shape, generator=gg, device=DEV)).to(dtype)
        s0, k0 = _counts()
        if fused:
            sb = utils.fused_step(comp, groups, names, shapes, nhp, {0: 1.0}, GAMMA, 0, defer_receive=defer,
                                  state=state)
            assert _counts()[0] - s0 == -(-len(lens) // CAP)
        else:
            utils.apply_gradient_loop(groups, state, True)
            sb = utils.fused_step(comp, groups, names, shapes, nhp, {0: 1.0}, GAMMA, 0, defer_receive=defer)
            assert _counts()[0] == s0
        rec = {"packs": _counts()[1] - k0, "x": _cat(params), "msg": _MESSAGE[op](sb).contiguous().view(torch.uint8).cpu().numpy().copy(),
               "bufs": _cat([state[p]["momentum_buffer"] for p in params])}
        if not defer:
            rec["hat"], rec["mem"] = host(nhp[0].buffer), host(nhp["memory"].buffer)
        out.append(rec)
    if defer:
        comp.flush_receive()
        out[-1]["hat"], out[-1]["mem"] = host(nhp[0].buffer), host(nhp["memory"].buffer)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("op,defer", [("compress_top_k", False), ("sign", False), ("sign", True)])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_fused_step_with_state_is_the_loop_then_todays_step(mode, op, defer):
    """ResNet-20's layout, three steps with weight decay and momentum, one rank (its own
    neighbourhood): utils.fused_step(state=...) against apply_gradient's per-tensor loop
    followed by today's fused_step -- x, x_hat, memory, the message and every momentum buffer."""
    a = _dropin_run(op, DTYPES[mode], defer, fused=True)
    b = _dropin_run(op, DTYPES[mode], defer, fused=False)
    for step, (ra, rb) in enumerate(zip(a, b)):
        assert ra.keys() == rb.keys()
        # recover_params' pack launch is gone, and only that one
        assert ra.pop("packs") == rb.pop("packs") - 1
        for key in ra:
            if key == "msg":
                assert ra[key].size > 0 and np.array_equal(ra[key], rb[key]), (step, key)
            else:
                assert same_bits(ra[key], rb[key]), (step, key)
    assert not same_bits(a[0]["x"], a[1]["x"]), "the params did not move"
