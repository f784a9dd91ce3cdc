"""Stochastic rounding for bf16 models on the device: choco_params_unpack_sr and
choco_params_sgd_sr bit for bit against the host restatement (utils.sr_bits / sr_narrow_bf16,
written from include/choco_codec.h) and utils.apply_gradient_sr_loop, on the 16-byte path and on
the element path; the rate; utils.fused_step(rounding=...); and the accumulation experiment."""
import collections

import numpy as np
import pytest
import torch

from chocosgd_amd import codec, utils

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
LENS = [1, 7, 8191, 8193, 0, 20000, 3]  # odd sizes, one past and one short of the 8192 tile, an empty tensor
DTYPES = [BF16, F32, BF16, BF16, F32, BF16, F32]
SEED = 5
STEPS = [0, 12345]


def _esz(dt):
    return 2 if dt == BF16 else 4


def _bits(t):
    """The bit patterns of a bf16 / fp32 tensor, on the host."""
    t = t.detach().reshape(-1).cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == BF16 else t.numpy().view(np.uint32)


def _eq(x, y, what):
    """Bit equality of two tensors; a mismatch prints how many elements differ before it fails."""
    a, b = _bits(x), _bits(y)
    bad = int((a != b).sum()) if a.shape == b.shape else -1
    if bad:
        print(f"{what}: {bad} of {a.size} elements differ")
    assert bad == 0, what


def _views(lens, dtypes, shift):
    """One tensor per entry, each a view into a byte buffer of its own.  shift 0: the address is
    congruent with the flat side modulo 16 bytes (q - esz * o0 = 0 mod 16: whole groups of 8 move
    as 16-byte vectors); shift 1: one element further (the element path)."""
    out, o0 = [], 0
    for m, dt in zip(lens, dtypes):
        esz = _esz(dt)
        store = torch.zeros(esz * m + 64, dtype=torch.uint8, device=DEV)
        assert store.data_ptr() % 16 == 0
        off = (esz * o0) % 16 + esz * shift
        t = store[off:off + esz * m].view(dt)
        assert t.numel() == m and (m == 0 or (t.data_ptr() - esz * o0) % 16 == (esz * shift) % 16)
        out.append(t)
        o0 += m
    return out


def _expected_unpack(flat, lens, dtypes, step):
    """Per tensor: the restatement for bf16 (bit patterns), None for fp32."""
    want, o = [], 0
    for m, dt in zip(lens, dtypes):
        want.append(_bits(utils.sr_narrow_bf16(flat[o:o + m], utils.sr_bits(SEED, step, o, m))) if dt == BF16 else None)
        o += m
    return want


@pytest.fixture(scope="module")
def flat_in():
    g = torch.Generator(device=DEV).manual_seed(3)
    n = sum(LENS)
    x = torch.randn(n, generator=g, device=DEV) * torch.exp2(torch.randint(-12, 12, (n,), generator=g, device=DEV).float())
    return x.contiguous()


@pytest.fixture(scope="module")
def plain_unpacked(flat_in):
    outs = _views(LENS, DTYPES, 0)
    codec.params_unpack(flat_in, outs)
    return [o.clone() for o in outs]


@pytest.fixture(scope="module")
def want_unpacked(flat_in):
    return {step: _expected_unpack(flat_in, LENS, DTYPES, step) for step in STEPS}


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("shift", [0, 1], ids=["vector", "element"])
def test_unpack_is_the_restatement_on_both_paths(flat_in, plain_unpacked, want_unpacked, shift, step):
    outs = _views(LENS, DTYPES, shift)
    before = codec.launch_count("param_unpack_sr_kernel"), codec.launch_count("param_unpack_kernel")
    codec.params_unpack(flat_in, outs, sr=(SEED, step))
    assert codec.launch_count("param_unpack_sr_kernel") - before[0] == codec.params_launches(len(LENS)) == 1
    assert codec.launch_count("param_unpack_kernel") == before[1]
    for s, (o, want, plain) in enumerate(zip(outs, want_unpacked[step], plain_unpacked)):
        if want is None:
            assert np.array_equal(_bits(o), _bits(plain)), f"fp32 tensor {s} is not the plain unpack's"
        else:
            assert np.array_equal(_bits(o), want), f"bf16 tensor {s} differs from the restatement"
    moved = sum(int((_bits(o) != _bits(p)).sum()) for o, p, w in zip(outs, plain_unpacked, want_unpacked[step])
                if w is not None)
    assert moved > 1000  # it is not round-to-nearest


def test_unpack_steps_differ(want_unpacked):
    a, b = (np.concatenate([w for w in want_unpacked[step] if w is not None]) for step in STEPS)
    assert 0.2 < float((a != b).mean()) < 0.6


@pytest.mark.parametrize("step", STEPS)
def test_unpack_across_the_chunk_of_192_tensors(step):
    lens, dtypes = [2] * 200, [BF16 if i % 3 else F32 for i in range(200)]
    g = torch.Generator(device=DEV).manual_seed(4)
    flat = torch.randn(400, generator=g, device=DEV)
    outs = [torch.zeros(2, dtype=dt, device=DEV) for dt in dtypes]
    before = codec.launch_count("param_unpack_sr_kernel")
    codec.params_unpack(flat, outs, sr=(SEED, step))
    assert codec.launch_count("param_unpack_sr_kernel") - before == codec.params_launches(200) == 2
    want = _expected_unpack(flat, lens, dtypes, step)
    for s, (o, w) in enumerate(zip(outs, want)):
        if w is None:
            assert torch.equal(o, flat[2 * s:2 * s + 2]), s
        else:
            assert np.array_equal(_bits(o), w), s


def test_unpack_special_values():
    bits = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC01234, 0x7F800001,  # 0, inf, NaN
                     0x3F800000, 0xBF810000, 0x7F7F0000, 0x00010000, 0x80400000,                          # bf16-exact
                     0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000,                                                  # largest finite
                     0x00000001, 0x00012345, 0x807FFFFF, 0x0000FFFF, 0x3FFFFFFF, 0xBFFFFFFF], dtype=np.uint32)
    bits = np.tile(bits, 40)  # every value meets many r16, in whole groups and in a cut one
    flat = torch.from_numpy(bits.view(np.float32).copy()).to(DEV)
    for shift in (0, 1):
        out = _views([bits.size], [BF16], shift)[0]
        codec.params_unpack(flat, [out], sr=(SEED, 7))
        got = _bits(out)
        want = _bits(utils.sr_narrow_bf16(flat, utils.sr_bits(SEED, 7, 0, bits.size)))
        assert np.array_equal(got, want)
        exact = (bits & 0xFFFF) == 0
        mag = bits & 0x7FFFFFFF
        assert np.array_equal(got[exact & (mag <= 0x7F800000)], (bits >> 16)[exact & (mag <= 0x7F800000)])
        assert np.all(got[mag > 0x7F800000] == 0x7FC0)
        up = got[bits == 0x7F7FFFFF]
        assert set(up.tolist()) <= {0x7F7F, 0x7F80} and 0x7F80 in up.tolist()  # may round to inf, as rounding up does


def test_unpack_rate_is_low16_over_65536():
    """1.0 plus a quarter of a bf16 ulp: the upper neighbour is taken by a quarter of the elements,
    0.25 +- 6 sigma with sigma = sqrt(0.25 * 0.75 / 2^20) = 4.2e-4; two steps agree where both or
    neither round up, so they differ in 2 * 0.25 * 0.75 = 0.375 of the elements."""
    n = 1 << 20
    flat = torch.from_numpy(np.full(n, 0x3F804000, dtype=np.uint32).view(np.float32)).to(DEV)
    outs = []
    for step in (0, 1):
        out = torch.zeros(n, dtype=BF16, device=DEV)
        codec.params_unpack(flat, [out], sr=(SEED, step))
        got = _bits(out)
        assert set(np.unique(got).tolist()) == {0x3F80, 0x3F81}
        frac = float((got == 0x3F81).mean())
        print(f"step {step}: fraction rounded up {frac:.5f}")
        assert abs(frac - 0.25) <= 0.0025, frac
        outs.append(got)
    assert np.array_equal(outs[0], _bits(utils.sr_narrow_bf16(flat, utils.sr_bits(SEED, 0, 0, n))))
    differ = float((outs[0] != outs[1]).mean())
    print(f"the two steps differ in {differ:.5f}")
    assert abs(differ - 0.375) <= 0.01, differ


def test_unpack_refuses_fp16():
    flat = torch.zeros(8, device=DEV)
    outs = [torch.zeros(4, dtype=BF16, device=DEV), torch.ones(4, dtype=torch.float16, device=DEV)]
    with pytest.raises(RuntimeError, match="tensor 1: fp16"):
        codec.params_unpack(flat, outs, sr=(SEED, 0))
    assert float(outs[1].sum()) == 4.0


# ----------------------------------------------------------------------------- the update
MODEL_LENS = [1, 7, 8191, 8193, 20000, 3]
MODEL_DTYPES = [BF16, F32, BF16, BF16, BF16, F32]
NOGRAD = 3
CONFIGS = {
    "plain": dict(weight_decay=0.0, momentum=0.0, dampening=0.0, nesterov=False),
    "wd": dict(weight_decay=5e-3, momentum=0.0, dampening=0.0, nesterov=False),
    "momentum_dampening": dict(weight_decay=5e-3, momentum=0.9, dampening=0.1, nesterov=False),
    "nesterov": dict(weight_decay=0.0, momentum=0.9, dampening=0.0, nesterov=True),
}
PINNED_TOTAL = 16.5  # about the gradients' norm: a pinned total makes the coefficient the same on both sides


def _model(values, shift, hp, lr=0.05):
    params = []
    for v, view in zip(values, _views(MODEL_LENS, MODEL_DTYPES, shift)):
        view.copy_(v)
        params.append(torch.nn.Parameter(view))
    groups = [dict(hp, params=[p], lr=lr) for p in params]
    return params, groups


def _set_grads(params, grads, shift):
    for i, (p, gv, view) in enumerate(zip(params, grads, _views(MODEL_LENS, MODEL_DTYPES, shift))):
        if i == NOGRAD:
            p.grad = None
        else:
            view.copy_(gv)
            p.grad = view


def _congruent_buffers(params, state, shift):
    """Rebind every momentum buffer to a view laid out as the parameters are (the first step's
    buffers are fresh allocations, whatever their tensor's flat offset)."""
    views = _views(MODEL_LENS, MODEL_DTYPES, shift)
    for p, view in zip(params, views):
        if "momentum_buffer" in state.get(p, {}):
            view.copy_(state[p]["momentum_buffer"])
            state[p]["momentum_buffer"] = view


@pytest.fixture(scope="module")
def model_values():
    g = torch.Generator(device=DEV).manual_seed(11)
    p0 = [torch.randn(m, generator=g, device=DEV).to(dt) for m, dt in zip(MODEL_LENS, MODEL_DTYPES)]
    grads = [[(0.1 * torch.randn(m, generator=g, device=DEV)).to(dt) for m, dt in zip(MODEL_LENS, MODEL_DTYPES)]
             for _ in range(2)]
    return p0, grads


@pytest.mark.parametrize("write", [True, False], ids=["written", "not_written"])
@pytest.mark.parametrize("clip", [None, 1.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("shift", [0, 1], ids=["vector", "element"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_update_is_the_loop_bit_for_bit(model_values, config, shift, clip, write):
    """Two steps (the first creates the momentum buffers) of the kernel (a), of
    apply_gradient_sr_loop on the same device tensors (b) and of the plain kernel started from
    (a)'s parameters at each step (c): parameters and flat against the loop, momentum buffers and
    fp32 tensors against the plain kernel."""
    p0, grads = model_values
    hp = CONFIGS[config]
    n = sum(MODEL_LENS)
    clip_t = None if clip is None else (clip, False, PINNED_TOTAL)
    models = [_model(p0, shift, hp) for _ in range(3)]
    states = [collections.defaultdict(dict) for _ in range(3)]
    (pa, ga), (pb, gb), (pc, gc) = models
    for step in range(2):
        for params, _ in models:
            _set_grads(params, grads[step], shift)
        for p, q in zip(pa, pc):
            q.data.copy_(p.data)
        flats = [torch.full((n,), float("nan"), device=DEV) for _ in range(3)]
        before = codec.launch_count("param_sgd_sr_kernel"), codec.launch_count("param_sgd_kernel")
        entries = [(g, g["params"][0]) for g in ga]
        assert utils._sgd_batched(entries, states[0], True, flats[0], write=write, clip=clip_t, sr=(SEED, step))
        assert codec.launch_count("param_sgd_sr_kernel") - before[0] == codec.params_sgd_launches(len(pa)) == 1
        assert codec.launch_count("param_sgd_kernel") == before[1]
        utils.apply_gradient_sr_loop(gb, states[1], SEED, step, clip_t, flats[1], write=write)
        entries = [(g, g["params"][0]) for g in gc]
        assert utils._sgd_batched(entries, states[2], True, flats[2], write=True, clip=clip_t)
        for i, (a, b, c) in enumerate(zip(pa, pb, pc)):
            _eq(a, b, (step, i, "parameter"))
            assert np.array_equal(_bits(a.grad), _bits(grads[step][i])) if i != NOGRAD else a.grad is None
            if a.dtype == F32 and write:
                _eq(a, c, (step, i, "an fp32 tensor is not the plain kernel's"))
            if not write or i == NOGRAD:
                want = p0[i]
                _eq(a, want, (step, i, "written without WRITE_PARAMS"))
            if hp["momentum"] != 0 and i != NOGRAD:
                ba, bb, bc = (s[p]["momentum_buffer"] for s, p in zip(states, (a, b, c)))
                _eq(ba, bb, (step, i, "momentum buffer against the loop"))
                if write or step == 0:  # (c) started from (a)'s parameters
                    _eq(ba, bc, (step, i, "momentum buffer against the plain kernel"))
            else:
                assert "momentum_buffer" not in states[0].get(a, {})
        _eq(flats[0], flats[1], (step, "flat is not the loop's unrounded p_new"))
        assert not bool(torch.isnan(flats[0]).any())
        if write:
            # flat is unrounded, and the stored bf16 parameter is its rounding with the bits of the flat index
            o = 0
            for a in pa:
                m = a.numel()
                if a.dtype == BF16:
                    want = _bits(utils.sr_narrow_bf16(flats[0][o:o + m], utils.sr_bits(SEED, step, o, m)))
                    assert np.array_equal(_bits(a), want)
                o += m
            off_grid = (_bits(flats[0]) & 0xFFFF) != 0
            assert float(off_grid.mean()) > 0.5
        for params, st in zip((pa, pb, pc), states):
            _congruent_buffers(params, st, shift)


def test_run_refuses_what_has_no_stochastic_form(model_values):
    p0, grads = model_values
    params, groups = _model(p0, 0, CONFIGS["plain"])
    _set_grads(params, grads[0], 0)
    params[NOGRAD].grad = torch.zeros_like(params[NOGRAD].data)
    plan = utils._sgd_fill([(g, g["params"][0]) for g in groups], collections.defaultdict(dict), True, None)
    flat = torch.zeros(sum(MODEL_LENS), device=DEV)
    with pytest.raises(RuntimeError, match="apply mode"):
        plan.run(flat, grad_mode=True, sr=(SEED, 0))
    with pytest.raises(RuntimeError, match="loss-scaled"):
        plan.run(flat, scaled=torch.zeros(4, device=DEV), sr=(SEED, 0))
    with pytest.raises(RuntimeError, match="norms"):
        plan.run(flat, norms=torch.zeros(len(params), device=DEV), clip_threshold=1.0, sr=(SEED, 0))
    half = [torch.nn.Parameter(torch.ones(8, dtype=torch.float16, device=DEV))]
    half[0].grad = torch.ones_like(half[0].data)
    gh = [dict(CONFIGS["plain"], params=half, lr=0.1)]
    with pytest.raises(RuntimeError, match="float16"):
        utils.apply_gradient(gh, collections.defaultdict(dict), rounding=(SEED, 0))
    plan16 = utils._sgd_fill([(gh[0], half[0])], collections.defaultdict(dict), True, None)
    with pytest.raises(RuntimeError, match="tensor 0: fp16"):
        plan16.run(None, sr=(SEED, 0))
    assert float(half[0].detach().sum()) == 8.0 and all(np.array_equal(_bits(p), _bits(v)) for p, v in zip(params, p0))


# ----------------------------------------------------------------------------- the CHOCO step
class _Loopback:
    def _agg(self, data, op, force_wait=False):
        return [], {0: data}

    def complete_wait(self, reqs):
        pass


@pytest.mark.parametrize("op", ["compress_top_k", "sign"])
def test_fused_step_rounds_each_parameter_once(op):
    """One rank, its own neighbourhood.  The model after the step is the stochastic rounding of the
    flat x the step ends with; a tensor with a zero gradient whose memory equals its x_hat is left
    on the bf16 grid by the step and is unchanged."""
    from chocosgd_amd.parallel_choco import CHOCOCompressor
    from chocosgd_amd.tensor_buffer import TensorBuffer
    lens, dtypes, still = [37, 4096, 5, 8195], [BF16, BF16, F32, BF16], 3
    n = sum(lens)
    g = torch.Generator(device=DEV).manual_seed(21)
    params = [torch.nn.Parameter(torch.randn(m, generator=g, device=DEV).to(dt)) for m, dt in zip(lens, dtypes)]
    for i, p in enumerate(params):
        p.grad = torch.zeros_like(p.data) if i == still else (0.1 * torch.randn(p.shape, generator=g, device=DEV)).to(p.dtype)
    groups = [{"params": [p], "name": f"p{i}", "lr": 0.05, "weight_decay": 0.0, "momentum": 0.9, "dampening": 0.0,
               "nesterov": False} for i, p in enumerate(params)]
    names = list(enumerate(gr["name"] for gr in groups))
    shapes = [(torch.Size([m]), m) for m in lens]
    sizes = [(m,) for m in lens]
    hat = torch.cat([p.detach().float() for p in params]) + 0.1 * torch.randn(n, generator=g, device=DEV)
    mem = hat + 0.05 * torch.randn(n, generator=g, device=DEV)
    o_still = sum(lens[:still])
    mem[o_still:o_still + lens[still]] = hat[o_still:o_still + lens[still]]
    nhp = {0: TensorBuffer.from_flat(hat, sizes), "memory": TensorBuffer.from_flat(mem, sizes)}
    comp = CHOCOCompressor(aggregator=_Loopback(), comm_op=op, comm_device="gpu", compress_ratio=0.9,
                           quantize_level=4, is_biased=False, backend="nccl", use_ipc=False)
    before = [p.data.clone() for p in params]
    sr = utils.StochasticRounding(SEED)
    names_k = ["param_sgd_sr_kernel", "param_unpack_sr_kernel", "param_sgd_kernel", "param_unpack_kernel",
               "param_pack_kernel"]
    k0 = [codec.launch_count(k) for k in names_k]
    sb = utils.fused_step(comp, groups, names, shapes, nhp, {0: 1.0}, 0.9, 0, state=collections.defaultdict(dict),
                          rounding=sr)
    assert [codec.launch_count(k) - c for k, c in zip(names_k, k0)] == [1, 1, 0, 0, 0]
    assert sr.state_dict() == {"seed": SEED, "step": 1}  # one next() served the update and the unpack
    x = sb["flatten_params"].buffer
    o = 0
    for i, (p, m) in enumerate(zip(params, lens)):
        if p.dtype == BF16:
            want = _bits(utils.sr_narrow_bf16(x[o:o + m], utils.sr_bits(SEED, 0, o, m)))
            assert np.array_equal(_bits(p), want), i
        else:
            assert torch.equal(p.data, x[o:o + m]), i
        o += m
    assert np.array_equal(_bits(params[still]), _bits(before[still])), "a bf16-exact parameter moved"
    assert not np.array_equal(_bits(params[1]), _bits(before[1]))
    # the flat x the step worked on was never rounded (the still tensor, at the end, is on the grid by construction)
    assert float(((_bits(x[:o_still]) & 0xFFFF) != 0).mean()) > 0.5


# ----------------------------------------------------------------------------- what it is for
def test_small_updates_survive_on_the_device():
    """4096 bf16 parameters at 1.0, g = 1.0, lr = 2^-12, 256 steps of one workgroup each: the plain
    kernel loses every update; with stochastic rounding the mean is within 6 sigma (1.5e-3) of
    1 - 256 * 2^-12 = 0.9375, and every element is the host loop's."""
    n, steps, lr = 4096, 256, 2.0 ** -12

    def model(dev):
        p = torch.nn.Parameter(torch.ones(n, dtype=BF16, device=dev))
        p.grad = torch.ones(n, dtype=BF16, device=dev)
        return p, [{"params": [p], "lr": lr, "weight_decay": 0.0, "momentum": 0.0, "dampening": 0.0, "nesterov": False}]

    p, groups = model(DEV)
    state = collections.defaultdict(dict)
    k0 = codec.launch_count("param_sgd_kernel")
    for _ in range(steps):
        utils.apply_gradient(groups, state)
    assert codec.launch_count("param_sgd_kernel") - k0 == steps
    assert torch.equal(p.data, torch.ones(n, dtype=BF16, device=DEV))  # every update was lost

    sr = utils.StochasticRounding(SEED)
    k0 = codec.launch_count("param_sgd_sr_kernel")
    for _ in range(steps):
        utils.apply_gradient(groups, state, rounding=sr)
    assert codec.launch_count("param_sgd_sr_kernel") - k0 == steps
    mean = float(p.data.double().mean())
    print(f"mean after {steps} steps: {mean:.5f}")
    assert abs(mean - 0.9375) <= 1.5e-3, mean

    q, groups_q = model("cpu")
    for step in range(steps):
        utils.apply_gradient_sr_loop(groups_q, state, SEED, step)
    assert np.array_equal(_bits(p), _bits(q))
