"""The batched parameter bridge on the device: codec.params_pack / params_unpack
(csrc/params.hip) and the layers above them (tensor_buffer.flatten / TensorBuffer,
utils.recover_params, utils.fused_step on a half-precision model).

Oracle: torch's own converting copy on the device, `t.float()` (exact widening) and
`t.to(dtype)` (round to nearest even), compared bit for bit on widened values."""
import numpy as np
import pytest
import torch

from conftest import golden_json, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
GAMMA = 0.9
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SENTINEL = -7.0  # exact in every dtype


def host(t):
    return t.detach().float().cpu().numpy()


def _layouts():
    return {
        "one": [1],
        "small": [1, 2, 3, 7, 8, 9, 31, 33],
        "tile_edge": [4095, 4096, 4097],
        "zeros": [0, 5, 0, 0, 11],
        "big_odd": [2 ** 20 + 3, 5, 64],
        "many": [1 + i % 13 for i in range(400)],  # 3 launches, chunk boundaries inside a tile
        "resnet20": golden_json("layouts.json")["resnet20_cifar10"],
    }


def _dtype_of(mode, i):
    return DTYPES[mode] if mode != "mixed" else list(DTYPES.values())[i % 3]


def _wide_randn(n, seed):
    """fp32 values over ~12 decades: past fp16's range at both ends, off every 16-bit grid."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(n, generator=g, device=DEV) * torch.pow(10.0, torch.rand(n, generator=g, device=DEV) * 12 - 7)


def _tensors(lens, mode, seed):
    """Each tensor its own allocation."""
    return [_wide_randn(m, seed + i).to(_dtype_of(mode, i)) for i, m in enumerate(lens)]


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16", "mixed"])
@pytest.mark.parametrize("layout", sorted(_layouts()))
def test_pack_and_unpack_match_torch(layout, mode):
    from chocosgd_amd import codec
    lens = _layouts()[layout]
    n = sum(lens)
    ts = _tensors(lens, mode, 100)
    flat = torch.full((n,), SENTINEL, device=DEV)
    codec.params_pack(ts, flat)
    want = torch.cat([t.float().view(-1) for t in ts])
    assert same_bits(host(flat), host(want)), "pack"

    src = _wide_randn(n, 7)
    outs = [torch.full_like(t, SENTINEL) for t in ts]
    codec.params_unpack(src, outs)
    off = 0
    for i, (o, m) in enumerate(zip(outs, lens)):
        assert o.dtype == ts[i].dtype
        assert same_bits(host(o), host(src[off:off + m].to(o.dtype))), f"unpack tensor {i}"
        off += m


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16", "mixed"])
def test_tensor_buffer_takes_the_batched_path_with_the_loops_bits(mode):
    """flatten / TensorBuffer / unpack: the same bits as the per-tensor loop (written out here)."""
    from chocosgd_amd.tensor_buffer import TensorBuffer, flatten
    lens = [37, 4096, 5, 0, 129]
    ts = [t.view(-1, 1) if i == 1 else t for i, t in enumerate(_tensors(lens, mode, 40))]
    n = sum(lens)
    tb = TensorBuffer(ts, dtype=torch.float32)
    loop = torch.empty(n, device=DEV)
    off = 0
    for t in ts:
        loop[off:off + t.numel()] = t.data.view(-1)
        off += t.numel()
    assert tb.buffer.dtype == torch.float32 and torch.equal(tb.buffer.view(torch.int32), loop.view(torch.int32))
    assert torch.equal(flatten(ts, dtype=torch.float32).view(torch.int32), loop.view(torch.int32))
    assert flatten(ts).dtype == ts[0].dtype  # dtype=None: today's rule
    tb.buffer.copy_(_wide_randn(n, 41))
    outs, outs_loop = [torch.zeros_like(t) for t in ts], [torch.zeros_like(t) for t in ts]
    tb.unpack(outs)
    for t, entry in zip(outs_loop, tb):
        t.data[:] = entry
    for a, b in zip(outs, outs_loop):
        assert same_bits(host(a), host(b))


def _guarded_views(lens, dtype, seed, gap):
    """Views into ONE storage: `gap` sentinel elements, then each tensor followed by `gap`
    sentinels.  gap = 1: every view is only element-aligned.  Returns (storage, views, mask of
    guard positions)."""
    total = gap + sum(m + gap for m in lens)
    store = torch.full((total,), SENTINEL, device=DEV, dtype=dtype)
    guard = torch.ones(total, dtype=torch.bool, device=DEV)
    views, p = [], gap
    for i, m in enumerate(lens):
        store[p:p + m] = _wide_randn(m, seed + i).to(dtype)
        guard[p:p + m] = False
        views.append(store[p:p + m])
        p += m + gap
    return store, views, guard


@pytest.mark.parametrize("flat_shift", [1, 4])
@pytest.mark.parametrize("gap", [1, 8])
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_alignment_and_neighbours(mode, gap, flat_shift):
    """Views at element alignment (gap 1) or 16-byte steps (gap 8) inside one storage, the
    flat buffer a slice at 4-byte (shift 1) or 16-byte (shift 4) alignment of a larger one:
    every guard keeps its sentinel after pack and after unpack, and the data match torch."""
    from chocosgd_amd import codec
    dtype = DTYPES[mode]
    lens = [1, 2, 3, 7, 8, 9, 31, 33, 4097, 16, 8200, 20]
    n = sum(lens)
    store, views, guard = _guarded_views(lens, dtype, 60, gap)
    before = store.clone()
    big = torch.full((n + 2 * flat_shift,), SENTINEL, device=DEV)
    flat = big[flat_shift:flat_shift + n]
    codec.params_pack(views, flat)
    assert torch.all(big[:flat_shift] == SENTINEL) and torch.all(big[flat_shift + n:] == SENTINEL)
    assert same_bits(host(flat), host(torch.cat([v.float() for v in views])))
    assert same_bits(host(store), host(before)), "pack wrote to its sources"

    big[flat_shift:flat_shift + n] = _wide_randn(n, 61)
    src = big.clone()
    codec.params_unpack(flat, views)
    assert same_bits(host(big), host(src)), "unpack wrote to the flat buffer"
    assert torch.all(store[guard] == SENTINEL), "a guard element was overwritten"
    off = 0
    for i, (v, m) in enumerate(zip(views, lens)):
        assert same_bits(host(v), host(flat[off:off + m].to(dtype))), f"tensor {i}"
        off += m


def test_adjacent_views_keep_their_neighbours():
    """Views packed next to each other in one storage, congruent with the flat side (the
    16-byte vector path): unpacking one chunk of tensors leaves the others' bytes alone."""
    from chocosgd_amd import codec
    lens = [3, 5, 8, 24, 1, 7, 4096, 13, 3, 32]
    n = sum(lens)
    for dtype in DTYPES.values():
        store = torch.full((n + 16,), SENTINEL, device=DEV, dtype=dtype)
        offs = np.concatenate([[0], np.cumsum(lens)])
        views = [store[8 + offs[i]:8 + offs[i + 1]] for i in range(len(lens))]
        src = _wide_randn(n, 70)
        # every other tensor only (as its own layout): the tensors between keep the sentinel
        for i in range(0, len(lens), 2):
            codec.params_unpack(src[offs[i]:offs[i + 1]].clone(), [views[i]])
        want = torch.full_like(store, SENTINEL)
        for i in range(0, len(lens), 2):
            want[8 + offs[i]:8 + offs[i + 1]] = src[offs[i]:offs[i + 1]].to(dtype)
        assert same_bits(host(store), host(want)), dtype
        codec.params_unpack(src, views)
        want[8:8 + n] = src.to(dtype)
        assert same_bits(host(store), host(want)), dtype


def _narrowing_patterns():
    f = lambda v: int(np.float32(v).view(np.uint32))  # noqa: E731
    pats = [
        0x3F808000, 0x3F818000,  # bf16 ties: to even downwards, to even upwards
        0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,  # just off the ties
        0x3F801000, 0x3F803000, 0x3F801001, 0x3F800FFF,  # fp16 ties (13 dropped bits) and off them
        0x7F7FFFFF, 0xFF7FFFFF,  # largest finite fp32: inf in both
        f(65504.0), 0x477FEFFF, f(65520.0), f(-65520.0), 0x477FF001,  # fp16 max, below / at / above the overflow tie
        f(2.0 ** -24), f(2.0 ** -25), 0x33000001, f(-2.0 ** -25), f(1.5 * 2.0 ** -24), f(2.5 * 2.0 ** -24),
        f(2.0 ** -14), 0x387FC000, 0x387FE000, 0x387FFFFF,  # fp16 normal / subnormal boundary
        0x00000000, 0x80000000, 0x7F800000, 0xFF800000,  # +-0, +-inf
        0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x7F80FFFF,  # NaNs, quiet and signalling payloads
        0x00000001, 0x00012345, 0x80400000, 0x00008000, 0x00018000,  # fp32 subnormals (bf16 subnormal ties)
        f(1.0), f(-1.0), f(3.14159265), f(1e-8), f(-1e30),
    ]
    while len(pats) % 8:
        pats.append(f(0.1 * len(pats)))
    return np.array(pats, dtype=np.uint32)


@pytest.mark.parametrize("shift", [0, 1])
def test_narrowing_table(shift):
    """Hand-picked fp32 bit patterns through unpack, on the vector path (shift 0: every
    group whole and aligned) and element by element (shift 1), against t.to(dtype)."""
    from chocosgd_amd import codec
    pats = _narrowing_patterns()
    m = len(pats)
    one = torch.from_numpy(pats.view(np.int32)).to(DEV).view(torch.float32)
    big = torch.zeros(2 * m + shift, device=DEV)
    flat = big[shift:]
    flat.copy_(torch.cat([one, one]))
    outs = [torch.zeros(m, device=DEV, dtype=torch.bfloat16), torch.zeros(m, device=DEV, dtype=torch.float16)]
    codec.params_unpack(flat, outs)
    for o in outs:
        want = one.to(o.dtype)
        got_bits, want_bits = o.view(torch.int16).cpu().numpy(), want.view(torch.int16).cpu().numpy()
        nan = torch.isnan(want).cpu().numpy()
        assert np.array_equal(torch.isnan(o).cpu().numpy(), nan), o.dtype
        bad = np.nonzero((got_bits != want_bits) & ~nan)[0]
        assert bad.size == 0, (o.dtype, [(hex(pats[i]), hex(got_bits[i] & 0xFFFF), hex(want_bits[i] & 0xFFFF))
                                         for i in bad])
    # and the way back is exact
    back = torch.zeros(2 * m, device=DEV)
    codec.params_pack(outs, back)
    assert same_bits(host(back), host(torch.cat([o.float() for o in outs])))


@pytest.mark.parametrize("layout", ["step", "many"])
def test_the_batched_path_ran(layout):
    from chocosgd_amd import codec
    from chocosgd_amd.tensor_buffer import TensorBuffer
    lens = {"step": [37, 4096, 5], "many": _layouts()["many"]}[layout]
    ts = _tensors(lens, "bf16", 80)
    per_call = codec.lib().choco_params_launches(len(lens))
    assert per_call == {"step": 1, "many": 3}[layout]
    p0, u0 = codec.launch_count("param_pack_kernel"), codec.launch_count("param_unpack_kernel")
    tb = TensorBuffer(ts, dtype=torch.float32)
    assert codec.launch_count("param_pack_kernel") - p0 == per_call
    assert codec.launch_count("param_unpack_kernel") == u0
    tb.unpack(ts)
    tb.unpack(ts)
    assert codec.launch_count("param_unpack_kernel") - u0 == 2 * per_call
    assert codec.launch_count("param_pack_kernel") - p0 == per_call


def test_non_contiguous_tensors_are_refused():
    from chocosgd_amd import codec
    t = torch.zeros(4, 6, device=DEV).t()
    with pytest.raises(RuntimeError):
        codec.params_pack([t], torch.zeros(24, device=DEV))
    with pytest.raises(RuntimeError):
        codec.params_unpack(torch.zeros(24, device=DEV), [t])
    with pytest.raises(RuntimeError):  # lengths that do not add up to the flat buffer
        codec.params_pack([torch.zeros(5, device=DEV)], torch.zeros(6, device=DEV))


STEP_LENS = [37, 4096, 5]


def _model(dtype, seed=90):
    g = torch.Generator(device=DEV).manual_seed(seed)
    params = [torch.randn(m, generator=g, device=DEV).to(dtype) for m in STEP_LENS]
    groups = [{"params": [p], "name": f"p{i}"} for i, p in enumerate(params)]
    names = list(enumerate(gr["name"] for gr in groups))
    return params, groups, names


def test_recover_params_on_a_bf16_model():
    from chocosgd_amd import utils
    from chocosgd_amd.tensor_buffer import TensorBuffer
    params, groups, names = _model(torch.bfloat16)
    n = sum(STEP_LENS)
    hat = torch.randn(n, device=DEV)
    nhp = {0: TensorBuffer.from_flat(hat, [(m,) for m in STEP_LENS])}
    got, fp, fh = utils.recover_params(groups, names, 0, nhp, get_hat_params=True)
    assert all(a is b for a, b in zip(got, params))
    assert fp.buffer.dtype == torch.float32 and fh.buffer.dtype == torch.float32
    assert same_bits(host(fp.buffer), host(torch.cat([p.float() for p in params])))
    assert same_bits(host(fh.buffer), host(hat))
    assert fh.buffer.data_ptr() != hat.data_ptr() and fh.buffer.data_ptr() != fp.buffer.data_ptr()
    assert [tuple(fh[i].shape) for i in range(len(fh))] == [(m,) for m in STEP_LENS]
    got2, fp2 = utils.recover_params(groups, names, get_hat_params=False)
    assert fp2.buffer.dtype == torch.float32 and torch.equal(fp2.buffer, fp.buffer)


class _Loopback:
    def _agg(self, data, op, force_wait=False):
        return [], {0: data}

    def complete_wait(self, reqs):
        pass


_MESSAGE = {"compress_top_k": lambda sb: sb["wire_message"],
            "sign": lambda sb: sb["sign_message"],
            "quantize_qsgd": lambda sb: sb["flatten_updates"].buffer}


def _one_step(op, params, groups, names, hat0, mem0):
    from chocosgd_amd import utils
    from chocosgd_amd.parallel_choco import CHOCOCompressor
    from chocosgd_amd.tensor_buffer import TensorBuffer
    shapes = [(torch.Size([m]), m) for m in STEP_LENS]
    sizes = [(m,) for m in STEP_LENS]
    nhp = {0: TensorBuffer.from_flat(hat0.clone(), sizes), "memory": TensorBuffer.from_flat(mem0.clone(), sizes)}
    comp = CHOCOCompressor(aggregator=_Loopback(), comm_op=op, comm_device="gpu", compress_ratio=0.9,
                           quantize_level=4, is_biased=False, backend="nccl", use_ipc=False)
    torch.manual_seed(1234)
    sb = utils.fused_step(comp, groups, names, shapes, nhp, {0: 1.0}, GAMMA, 0)
    torch.cuda.synchronize()
    return sb, nhp


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("op", ["compress_top_k", "sign", "quantize_qsgd"])
def test_fused_step_on_a_half_precision_model(op, mode):
    """Run A: the step on half-precision params.  Run B: the same step on their fp32 widening,
    rounded to the model's dtype afterwards.  The consensus step, the delta and the message come
    from the unrounded fp32 copy (parallel_choco_v.py:116-152), so everything agrees bit for bit
    -- and x_hat moved, i.e. the gossip really ran (pipeline() only prints a RuntimeError)."""
    dtype = DTYPES[mode]
    n = sum(STEP_LENS)
    g = torch.Generator(device=DEV).manual_seed(91)
    hat0 = torch.randn(n, generator=g, device=DEV)
    mem0 = torch.randn(n, generator=g, device=DEV)

    pa, ga, na = _model(dtype)
    sb_a, nhp_a = _one_step(op, pa, ga, na, hat0, mem0)

    pb = [p.float() for p in _model(dtype)[0]]
    gb = [{"params": [p], "name": f"p{i}"} for i, p in enumerate(pb)]
    sb_b, nhp_b = _one_step(op, pb, gb, na, hat0, mem0)

    assert sb_a["flatten_params"].buffer.dtype == torch.float32
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert a.dtype == dtype
        assert same_bits(host(a), host(b.to(dtype))), f"param {i}"
    assert same_bits(host(nhp_a[0].buffer), host(nhp_b[0].buffer)), "x_hat"
    assert same_bits(host(nhp_a["memory"].buffer), host(nhp_b["memory"].buffer)), "memory"
    ma, mb = _MESSAGE[op](sb_a), _MESSAGE[op](sb_b)
    assert ma.dtype == mb.dtype and ma.numel() == mb.numel() > 0
    assert torch.equal(ma.contiguous().view(torch.uint8), mb.contiguous().view(torch.uint8)), "message"
    assert not torch.equal(nhp_a[0].buffer, hat0), "x_hat did not move: no gossip ran"
    x0 = torch.cat([p.float() for p in _model(dtype)[0]])
    assert not torch.equal(torch.cat([p.float() for p in pa]), x0), "the params did not move"
