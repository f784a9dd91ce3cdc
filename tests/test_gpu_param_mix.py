"""The neighbour-weighted model mix on the device: choco_params_mix through codec.params_mix /
ParamSgdPlan.mix, DecentralizedAggregation._agg(op="weighted") and the three steps built on it
(dcd.fused_step, ecd.fused_step, utils.dpsgd_step).

The fp32 fixtures are the reference's own results (tests/golden/mix_*.npz); every other kernel
case is checked against the numpy model (tests/_mix_oracle.py), and the steps against their
per-op torch paths run on CPU copies.  Everything is compared as bit patterns over whole
storages, so that every byte a launch does not own is checked together with the ones it does."""
import collections

import numpy as np
import pytest
import torch

from conftest import golden, same_bits
import _mix_oracle as MO
import _sgd_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SENTINEL = -7.0  # exact in every dtype
GAP = 64  # elements between two views of a storage: 64 * esz is a multiple of 16 bytes
SETS = ["ring3", "five", "one"]
LOCAL_INDEX = [1, 5]
SUB, FMA, WRITE, EXT = 1, 2, 4, 8  # CHOCO_MIX_*


def host(t):
    return t.detach().float().cpu().numpy()


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(dtype)


def _offs(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


class Views:
    """Tensors as views into ONE storage: view s starts at element GAP * (s + 1) + off_s + shift,
    so with shift 0 every view is congruent with the 16-byte group grid of the flat layout (the
    vector path) and with shift 1 none is (the scalar path); everything between is sentinel."""

    def __init__(self, flat, lens, dtype, shift=0):
        self.lens = list(lens)
        off = _offs(lens)
        self.starts = [GAP * (s + 1) + int(off[s]) + shift for s in range(len(lens))]
        self.total = GAP * (len(lens) + 2) + int(off[-1])
        self.store = torch.full((self.total,), SENTINEL, device=DEV, dtype=DTYPES[dtype])
        self.views = [self.store[a:a + m] for a, m in zip(self.starts, lens)]
        o = 0
        for v, m in zip(self.views, self.lens):
            v.copy_(dev(flat[o:o + m], v.dtype))
            o += m

    def expect(self, flat):
        """The whole storage as fp32 with `flat` in the views."""
        out = np.full(self.total, SENTINEL, dtype=np.float32)
        o = 0
        for a, m in zip(self.starts, self.lens):
            out[a:a + m] = flat[o:o + m]
            o += m
        return out

    def all(self):
        return host(self.store)


class Flat:
    """A flat fp32 buffer of n elements inside a sentinel storage, 16-byte aligned with shift 0."""

    def __init__(self, n, values=None, shift=0):
        self.n, self.a = n, 4 + shift
        self.store = torch.full((n + 12,), SENTINEL, device=DEV)
        self.t = self.store[self.a:self.a + n]
        if values is not None:
            self.t.copy_(dev(values))

    def expect(self, values):
        out = np.full(self.n + 12, SENTINEL, dtype=np.float32)
        out[self.a:self.a + self.n] = values
        return out

    def all(self):
        return host(self.store)


def _mix(plan, srcs, weights, nseg, **kw):
    """plan.mix with the launch count checked against choco_params_mix_launches."""
    from chocosgd_amd import codec
    c0 = codec.launch_count("param_mix_kernel")
    plan.mix([s.t for s in srcs], weights, **kw)
    assert codec.launch_count("param_mix_kernel") - c0 == codec.params_mix_launches(nseg, len(srcs))


def _plan(pv, gv):
    from chocosgd_amd import codec
    plan = codec.ParamSgdPlan(pv.views)
    for i, (p, g) in enumerate(zip(pv.views, gv.views)):
        plan.param_ptrs[i], plan.grad_ptrs[i] = p.data_ptr(), g.data_ptr()
    return plan


def _run_modes(p, d, srcs_np, weights, lens, lr, dtype, shift):
    """The three optimizers' launches on one layout against the numpy model; returns a dict of
    (got, want) pairs of whole storages.  p, d: values on the dtype's grid."""
    n, nseg = int(sum(lens)), len(lens)
    out = {}

    def fresh():
        pv, gv = Views(p, lens, dtype, shift), Views(d, lens, dtype, shift)
        srcs = [Flat(n, s, shift) for s in srcs_np]
        return pv, gv, srcs, _plan(pv, gv)

    def unchanged(tag, gv, srcs):
        out[f"{tag} grads"] = (gv.all(), gv.expect(d))
        for r, s in enumerate(srcs):
            out[f"{tag} source {r}"] = (s.all(), s.expect(srcs_np[r]))

    # DCD: half params and the packed params, nothing else written
    pv, gv, srcs, plan = fresh()
    half, xo = Flat(n, shift=shift), Flat(n, shift=shift)
    _mix(plan, srcs, weights, nseg, lr=lr, mode=SUB, flat_out=half.t, x_out=xo.t)
    _, _, want = MO.mix(srcs_np, weights, g=d, lr=lr, grad="sub", dtype=dtype)
    out["dcd half"] = (half.all(), half.expect(want))
    out["dcd packed"] = (xo.all(), xo.expect(p))
    out["dcd params"] = (pv.all(), pv.expect(p))
    unchanged("dcd", gv, srcs)
    # ECD: params written (narrowed), the extrapolation from the un-narrowed sum
    for t in LOCAL_INDEX:
        pv, gv, srcs, plan = fresh()
        ex = Flat(n, shift=shift)
        _mix(plan, srcs, weights, nseg, lr=lr, mode=FMA | WRITE | EXT, ext_a=1 - 0.5 * t, ext_b=0.5 * t, flat_out=ex.t)
        _, p_new, want = MO.mix(srcs_np, weights, g=d, lr=lr, grad="fma", x=p, ext=(1 - 0.5 * t, 0.5 * t), dtype=dtype)
        out[f"ecd{t} params"] = (pv.all(), pv.expect(p_new))
        out[f"ecd{t} extrap"] = (ex.all(), ex.expect(want))
        unchanged(f"ecd{t}", gv, srcs)
    # D-PSGD: the params alone
    pv, gv, srcs, plan = fresh()
    run = Flat(n, shift=shift) if len(srcs) > 8 else None  # the running sum of chained launches
    _mix(plan, srcs, weights, nseg, mode=WRITE, flat_out=run.t if run else None)
    m, p_new, _ = MO.mix(srcs_np, weights, dtype=dtype)
    out["dpsgd params"] = (pv.all(), pv.expect(p_new))
    if run:
        out["dpsgd flat"] = (run.all(), run.expect(m))
    unchanged("dpsgd", gv, srcs)
    return out


def _assert_all(pairs):
    for what, (got, want) in pairs.items():
        assert same_bits(got, want), what


# ----------------------------------------------------------------------------- the kernel
@pytest.fixture(scope="module")
def inputs():
    return golden("mix_inputs")


@pytest.mark.parametrize("name", SETS)
def test_fixtures_through_the_abi(inputs, name):
    """The reference's own results, fp32, vector path: DCD's half and packed params, ECD's params
    and extrapolated model at both local indices, D-PSGD's aggregate."""
    fx = golden(f"mix_{name}")
    rank, info = int(fx["rank"]), dict(zip(fx["ranks"].tolist(), fx["weights"].tolist()))
    lr, wd, mom, damp, nest = inputs["hp"].tolist()
    lens = inputs["lens"].tolist()
    p0 = inputs["p0"]
    p_sgd, _, d = SO.sgd_step(p0, inputs["g"], None, lr, wd, mom, damp, bool(nest), first=True)
    hats = [inputs["hats"][r] for r in info]
    w = list(info.values())
    pairs = _run_modes(p0, d, hats, w, lens, lr, "fp32", 0)
    _assert_all(pairs)
    # ... and the same storages against the fixtures themselves
    pv = Views(p0, lens, "fp32")
    n = len(p0)
    assert same_bits(pairs["dcd half"][0], Flat(n).expect(fx["dcd_half"]))
    assert same_bits(pairs["dcd packed"][0], Flat(n).expect(fx["dcd_packed"]))
    for t in LOCAL_INDEX:
        assert same_bits(pairs[f"ecd{t} params"][0], pv.expect(fx[f"ecd{t}_params"]))
        assert same_bits(pairs[f"ecd{t} extrap"][0], Flat(n).expect(fx[f"ecd{t}_extrap"]))
    # D-PSGD mixes what was exchanged: the neighbours first, this rank's updated params last
    order = [r for r in info if r != rank] + [rank]
    srcs = [p_sgd if r == rank else inputs["hats"][r] for r in order]
    pairs = _run_modes(p_sgd, d, srcs, [info[r] for r in order], lens, lr, "fp32", 0)
    _assert_all(pairs)
    assert same_bits(pairs["dpsgd params"][0], pv.expect(fx["dpsgd_agg"]))


def _layout_values(lens, seed, dtype, nsrc):
    rng = np.random.RandomState(seed)
    n = int(sum(lens))
    p = SO.to_grid((rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 1, n)).astype(np.float32), dtype)
    d = SO.to_grid((rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 0, n)).astype(np.float32), dtype)
    srcs = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 1, n)).astype(np.float32) for _ in range(nsrc)]
    return p, d, srcs


LAYOUT = [5, 1, 0, 8195, 33, 4099, 17000, 40, 40, 1]


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_views_inside_one_storage(dtype, shift):
    """The fixture layout as views of one storage, element-misaligned with shift 1 (the scalar
    path; flat buffers at 4-byte alignment too): the narrowing store, x_out as exact widening,
    the extrapolation from the un-narrowed sum; special values on both paths."""
    p, d, srcs = _layout_values(LAYOUT, 17, dtype, 3)
    o = int(_offs(LAYOUT)[3])
    for s in srcs:
        s[o + 11] = -0.0            # 0 + (-0 * w) = +0
        s[o + 4000] = 0.0
    srcs[0][o + 4000] = 2.0e-38     # a subnormal product
    srcs[1][o + 30], srcs[1][o + 5000] = np.inf, 7.0e4  # inf * 0 = NaN; past fp16's range
    d[o + 41] = np.nan
    d[o + 20], d[o + 21] = 0.0, -0.0
    _assert_all(_run_modes(p, d, srcs, [0.5, 0.0, 1.0 / 3], LAYOUT, 0.1, dtype, shift))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_many_small_tensors(dtype):
    """300 tensors of 1 to 40 elements: three launches that share one tile; every sentinel between
    two tensors and around the flat buffers stays."""
    from chocosgd_amd import codec
    rng = np.random.RandomState(5)
    lens = rng.randint(1, 41, 300).tolist()
    assert codec.params_mix_launches(len(lens), 3) == 3 and sum(lens) < 8192
    p, d, srcs = _layout_values(lens, 6, dtype, 3)
    for shift in (0, 1):
        _assert_all(_run_modes(p, d, srcs, [0.25, 0.5, 0.25], lens, 0.05, dtype, shift))


@pytest.mark.parametrize("nsrc", [1, 3, 8, 9, 17])
def test_source_counts(nsrc):
    """A 20,000-element flat buffer: more than 8 sources run as chained launches of 8 and equal
    the one sum bit for bit, alone and with a tail behind the last launch only."""
    from chocosgd_amd import codec
    n = 20000
    rng = np.random.RandomState(nsrc)
    srcs_np = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 1, n)).astype(np.float32) for _ in range(nsrc)]
    w = rng.uniform(0.0, 0.4, nsrc).tolist()
    for s in srcs_np:
        s[123] = -0.0
    srcs_np[-1][777] = np.inf
    if nsrc > 1:
        w[-1] = 0.0
    for shift in (0, 1):
        srcs = [Flat(n, s, shift) for s in srcs_np]
        out = Flat(n, shift=shift)
        c0 = codec.launch_count("param_mix_kernel")
        assert codec.params_mix([s.t for s in srcs], w, flat_out=out.t) is None
        assert codec.launch_count("param_mix_kernel") - c0 == codec.params_mix_launches(1, nsrc) == 1 + (nsrc - 1) // 8
        want = MO.weighted_sum(srcs_np, w)
        assert want.view(np.uint32)[123] == 0 and (np.isnan(want[777]) if nsrc > 1 else np.isinf(want[777]))
        assert same_bits(out.all(), out.expect(want))
        for s, v in zip(srcs, srcs_np):
            assert same_bits(s.all(), s.expect(v))
    lens = [8195, 11805]
    p, d, _ = _layout_values(lens, 40 + nsrc, "bf16", 0)
    _assert_all(_run_modes(p, d, srcs_np, w, lens, 0.1, "bf16", 0))


def test_weighted_aggregate_takes_the_kernel():
    """_agg(op="weighted") on ROCm tensors: one mix call, the bits of the CPU expression, the
    data's shape; other dtypes keep the expression."""
    from chocosgd_amd import codec
    rng = np.random.RandomState(8)
    info = {0: 1.0 / 3, 1: 1.0 / 3, 2: 1.0 / 3}
    cpu = {r: torch.from_numpy(rng.standard_normal((40, 251)).astype(np.float32)) for r in info}
    cpu[0][3, 7] = cpu[1][3, 7] = cpu[2][3, 7] = -0.0
    gpu = {r: t.to(DEV) for r, t in cpu.items()}
    want = MO.prepared_aggregator(1, info, cpu)._agg(cpu[1], op="weighted")
    c0 = codec.launch_count("param_mix_kernel")
    got = MO.prepared_aggregator(1, info, gpu)._agg(gpu[1], op="weighted")
    assert codec.launch_count("param_mix_kernel") - c0 == 1
    assert got.shape == want.shape and same_bits(host(got), want.numpy())
    assert all(torch.equal(gpu[r].cpu(), cpu[r]) for r in info)
    half = {r: t.half() for r, t in gpu.items()}
    got16 = MO.prepared_aggregator(1, info, half)._agg(half[1], op="weighted")
    assert codec.launch_count("param_mix_kernel") - c0 == 1 and got16.dtype == torch.float16


# ----------------------------------------------------------------------------- the steps
STEP_LENS = [5, 1, 8195, 33, 4099, 40]  # no empty tensor: the segmented top-k has no slot for one
INFO = {0: 0.25, 1: 0.5, 2: 0.25}
RANK = 1
HP = dict(lr=0.1, weight_decay=1e-4, momentum=0.9, dampening=0.0, nesterov=False)


class _Echo:
    """The exchange of a neighbourhood whose every rank sends what this rank sends."""

    def __init__(self, rank, ranks):
        self.rank, self.ranks = rank, list(ranks)

    def _agg(self, data, op, force_wait=True):
        assert op == "get_raw_sync_data" and force_wait
        return {r: data for r in self.ranks}


class _OnDevice:
    """The device compressor behind a CPU step: what compress is handed, and the replicas, are
    moved to the device for it and the replicas back."""

    def __init__(self, real):
        self.real, self.aggregator_fn = real, real.compressor_fn.aggregator_fn

    @staticmethod
    def _up(buf):
        from chocosgd_amd.tensor_buffer import TensorBuffer
        return TensorBuffer.from_flat(buf.buffer.to(DEV), buf._tensors_sizes)

    def compress(self, sync_buffer):
        self.sb = {k: self._up(v) if hasattr(v, "buffer") else v for k, v in sync_buffer.items()}
        self.real.compress(self.sb)
        sync_buffer["n_bits"] = self.sb["n_bits"]

    def sync(self, sync_buffer):
        self.real.sync(self.sb)

    def uncompress(self, sync_buffer, neighbor_hat_params, *local_index):
        up = {r: self._up(h) for r, h in neighbor_hat_params.items()}
        self.real.uncompress(self.sb, up, *local_index)
        for r, h in neighbor_hat_params.items():
            h.buffer.copy_(up[r].buffer)


def _step_model(p0, device):
    params = [torch.nn.Parameter(torch.from_numpy(p0[o:o + m].copy()).to(device))
              for o, m in zip(_offs(STEP_LENS)[:-1], STEP_LENS)]
    groups = [dict(HP, params=[p], name=f"p{i}") for i, p in enumerate(params)]
    names = list(enumerate(g["name"] for g in groups))
    shapes = [(p.size(), p.nelement()) for p in params]
    return params, groups, names, shapes, collections.defaultdict(dict)


def _set_grads(params, flat):
    for p, o, m in zip(params, _offs(STEP_LENS)[:-1], STEP_LENS):
        p.grad = torch.from_numpy(flat[o:o + m].copy()).to(p.device)


def _replicas(hats, device):
    from chocosgd_amd.tensor_buffer import TensorBuffer
    return {r: TensorBuffer.from_flat(torch.from_numpy(hats[r].copy()).to(device), [(m,) for m in STEP_LENS])
            for r in INFO}


def _cat(tensors):
    return np.concatenate([host(t).reshape(-1) for t in tensors])


def _step_inputs(seed):
    rng = np.random.RandomState(seed)
    n = sum(STEP_LENS)
    p0 = rng.standard_normal(n).astype(np.float32)
    gs = [(rng.standard_normal(n) * 0.1).astype(np.float32) for _ in range(2)]
    hats = {r: (p0 + rng.standard_normal(n) * 0.05).astype(np.float32) for r in INFO}
    return p0, gs, hats


def _compressor(module, comm_op):
    cls = module.DCDCompressor if module.__name__.endswith("dcd") else module.ECDCompressor
    return cls(aggregator=_Echo(RANK, INFO), comm_op=comm_op, comm_device="gpu", compress_ratio=0.9,
               quantize_level=4, is_biased=True, backend="nccl", use_ipc=False)


@pytest.mark.parametrize("comm_op", ["compress_top_k", "sign"])
@pytest.mark.parametrize("which", ["dcd", "ecd"])
def test_fused_steps_against_their_torch_paths(which, comm_op):
    """Two consecutive steps of dcd.fused_step / ecd.fused_step on the device against step_loop on
    CPU copies (with the same device compressor behind it): params, replicas and momentum
    buffers identical, one mix launch per step."""
    from chocosgd_amd import codec, dcd, ecd
    module = dcd if which == "dcd" else ecd
    p0, gs, hats = _step_inputs(3)
    pa, ga, na, sha, sa = _step_model(p0, DEV)
    pb, gb, nb, shb, sb = _step_model(p0, "cpu")
    ha, hb = _replicas(hats, DEV), _replicas(hats, "cpu")
    ca, cb = _compressor(module, comm_op), _OnDevice(_compressor(module, comm_op))
    for k in range(2):
        _set_grads(pa, gs[k])
        _set_grads(pb, gs[k])
        extra = () if which == "dcd" else (k + 2,)
        c0 = codec.launch_count("param_mix_kernel")
        bits_a = module.fused_step(ca, ga, na, sa, sha, ha, INFO, *extra)
        assert codec.launch_count("param_mix_kernel") - c0 == 1
        bits_b = module.step_loop(cb, gb, nb, sb, shb, hb, INFO, *extra)
        assert codec.launch_count("param_mix_kernel") - c0 == 1, "the torch path took the kernel"
        assert bits_a == bits_b
        assert same_bits(_cat(pa), _cat(pb)), f"params after step {k}"
        for r in INFO:
            assert same_bits(host(ha[r].buffer), host(hb[r].buffer)), f"replica {r} after step {k}"
        assert same_bits(_cat([sa[p]["momentum_buffer"] for p in pa]), _cat([sb[p]["momentum_buffer"] for p in pb]))
        assert same_bits(_cat([p.grad for p in pa]), _cat([p.grad for p in pb])), "d_p in the grads"
    assert not same_bits(_cat(pa), p0)


def test_dpsgd_step_against_its_torch_path():
    from chocosgd_amd import codec, utils
    p0, gs, hats = _step_inputs(4)
    pa, ga, na, _, sa = _step_model(p0, DEV)
    pb, gb, nb, _, sb = _step_model(p0, "cpu")
    recv = {r: torch.from_numpy(hats[r].copy()) for r in INFO if r != RANK}
    agg_a = MO.prepared_aggregator(RANK, INFO, {r: t.to(DEV) for r, t in recv.items()})
    agg_b = MO.prepared_aggregator(RANK, INFO, recv)
    for k in range(2):
        _set_grads(pa, gs[k])
        _set_grads(pb, gs[k])
        c0 = [codec.launch_count(nm) for nm in ("param_sgd_kernel", "param_mix_kernel", "param_unpack_kernel")]
        bits_a = utils.dpsgd_step(ga, na, sa, agg_a, INFO)
        c1 = [codec.launch_count(nm) for nm in ("param_sgd_kernel", "param_mix_kernel", "param_unpack_kernel")]
        assert [b - a for a, b in zip(c0, c1)] == [1, 1, 0], "one fused update + pack, one mix, no unpack"
        assert bits_a == utils.dpsgd_step_loop(gb, nb, sb, agg_b) == 32 * sum(STEP_LENS)
        assert same_bits(_cat(pa), _cat(pb)), f"params after step {k}"
        assert same_bits(_cat([sa[p]["momentum_buffer"] for p in pa]), _cat([sb[p]["momentum_buffer"] for p in pb]))
        assert same_bits(_cat([p.grad for p in pa]), gs[k]), "apply mode wrote the grads"
