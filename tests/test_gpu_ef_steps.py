"""deep_squeeze.fused_step and ef_sign.fused_step on the device: against the reference's own two
steps (tests/golden/ef_distinct_ds_topk.npz -- no ties in any top-k input --, ef_exact_ds_sign.npz
and ef_exact_efsign.npz -- norms that are the same bits in any summation order; gen_golden_ef.py)
bit for bit, and against step_loop, the reference's op sequence, on the same device for the
compressors whose draws are this codec's own (QSGD, random-k) and for a bf16 model.

One difference from the reference is by design and older than these steps (utils.apply_gradient):
in apply mode the gradient tensors are never written, where the reference adds the weight decay
into p.grad in place.  DeepSqueeze's p.grad is therefore compared with the gradient that was set
(the exact set has no weight decay, so there the two are the same thing); EF-signSGD's p.grad,
which the step does write, with the fixture's."""
import collections

import numpy as np
import pytest
import torch

from conftest import golden, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED0 = 5000  # torch.manual_seed(SEED0 + step) before each step: the seed random-k / QSGD draw
RANK, W = 1, 3
INFO = {r: 1.0 / W for r in range(W)}


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(dtype)


def host(t):
    return t.detach().float().cpu().numpy()


def _cat(tensors):
    return np.concatenate([host(t).reshape(-1) for t in tensors])


def _sizes(lens):
    return [torch.Size([m]) for m in lens]


def _split(flat, lens, dtype=torch.float32, device=DEV):
    out, o = [], 0
    for m in lens:
        out.append(torch.from_numpy(np.array(flat[o:o + m], dtype=np.float32)).to(device).to(dtype))  # a copy
        o += m
    return out


class _Model:
    def __init__(self, fx, dtype=torch.float32, device=DEV):
        from chocosgd_amd.tensor_buffer import TensorBuffer
        self.lens = fx["layout"].tolist()
        lr, wd, mom = fx["hp"].tolist()
        self.dtype, self.device = dtype, device
        self.params = [torch.nn.Parameter(t) for t in _split(fx["p0"], self.lens, dtype, device)]
        self.groups = [{"params": [p], "lr": lr, "weight_decay": wd, "momentum": mom, "dampening": 0.0,
                        "nesterov": False, "name": f"p{i}"} for i, p in enumerate(self.params)]
        self.names = list(enumerate(g["name"] for g in self.groups))
        self.shapes = [(p.size(), p.nelement()) for p in self.params]
        self.state = collections.defaultdict(dict)
        mem0 = torch.from_numpy(fx["mem0"].copy()).to(device)
        self.memory = TensorBuffer.from_flat(mem0, _sizes(self.lens))

    def set_grads(self, g):
        for p, gt in zip(self.params, _split(g, self.lens, self.dtype, self.device)):
            p.grad = gt

    def snapshot(self):
        return dict(params=_cat(self.params), mem=host(self.memory.buffer),
                    bufs=_cat([self.state[p]["momentum_buffer"] for p in self.params]),
                    grad=_cat([p.grad for p in self.params]))


class _Neighbours:
    """In the aggregators' place: this rank's own message with the neighbours' prepared ones."""

    def __init__(self):
        self.msgs, self.calls = {}, 0

    def _agg(self, data, op=None, force_wait=True, communication_scheme=None, async_op=False):
        self.calls += 1
        every = [data if r == RANK else self.msgs[r] for r in range(W)]
        return every if communication_scheme == "all_gather" else dict(enumerate(every))


class _Capture:
    def __init__(self):
        self.sent = []

    def _agg(self, data, op=None, force_wait=True, **kw):
        self.sent.append(data.clone())
        return {0: data}


def _ds_args(comm_op, gamma, q=4):
    return dict(comm_op=comm_op, comm_device="gpu", compress_ratio=0.9, quantize_level=q, is_biased=False,
                backend="nccl", use_ipc=False, consensus_stepsize=gamma)


def _ds_wires(fx, comm_op, q=4):
    """{step: {rank: wire}} of the two neighbours, made by this codec's compressors from the buffers
    the fixture says their compressors were handed (random-k / QSGD: seeded per rank and step)."""
    from chocosgd_amd.deep_squeeze import DeepSqueezeCompressor
    from chocosgd_amd.tensor_buffer import TensorBuffer
    lens = fx["layout"].tolist()
    shapes = [(torch.Size([m]), m) for m in lens]
    out = {}
    for t in (1, 2):
        out[t] = {}
        for j, r in enumerate((0, 2)):
            cap = _Capture()
            comp = DeepSqueezeCompressor(aggregator=cap, rank=r, **_ds_args(comm_op, float(fx["gamma"]), q))
            sb = {"original_shapes": shapes, "params_tb": TensorBuffer.from_flat(dev(fx["nbr"][t - 1, j]), _sizes(lens))}
            torch.manual_seed(SEED0 + 100 * t + r)
            comp.compress(sb)
            comp.sync(sb)
            out[t][r] = cap.sent[0]
    return out


def _ef_wires(fx):
    from chocosgd_amd.ef_sign import EFSignCompressor
    from chocosgd_amd.tensor_buffer import TensorBuffer
    lens = fx["layout"].tolist()
    out = {}
    for t in (1, 2):
        out[t] = {}
        for j, r in enumerate((0, 2)):
            comp = EFSignCompressor(rank=r, world_size=W, aggregator=None, comm_op="sign", comm_device="gpu",
                                    use_ipc=False)
            sb = comp.compress(TensorBuffer.from_flat(dev(fx["nbr"][t - 1, j]), _sizes(lens)))
            out[t][r] = sb["sign_message"].clone()
    return out


def _run_ds(fx, comm_op, wires, which, q=4, dtype=torch.float32, device=DEV):
    """Two steps of deep_squeeze.<which>; returns [(snapshot, n_bits)] and the aggregator."""
    from chocosgd_amd import deep_squeeze
    m = _Model(fx, dtype, device)
    nb = _Neighbours()
    comp = deep_squeeze.DeepSqueezeCompressor(aggregator=nb, rank=RANK, **_ds_args(comm_op, float(fx["gamma"]), q))
    out = []
    for t in (1, 2):
        m.set_grads(fx["g"][t - 1])
        nb.msgs = wires[t]
        torch.manual_seed(SEED0 + t)
        bits = getattr(deep_squeeze, which)(comp, m.groups, m.names, m.state, m.shapes, m.memory, INFO)
        out.append((m.snapshot(), bits))
    return out, nb


def _run_ef(fx, wires, which, dtype=torch.float32):
    from chocosgd_amd import ef_sign
    m = _Model(fx, dtype)
    nb = _Neighbours()
    comp = ef_sign.EFSignCompressor(rank=RANK, world_size=W, aggregator=nb, comm_op="sign", comm_device="gpu",
                                    use_ipc=False)
    out = []
    for t in (1, 2):
        m.set_grads(fx["g"][t - 1])
        nb.msgs = wires[t]
        bits = getattr(ef_sign, which)(comp, m.groups, m.names, m.state, m.memory)
        out.append((m.snapshot(), bits))
    return out, nb


def _assert_same_runs(a, b):
    for t, ((sa, ba), (sb, bb)) in enumerate(zip(a, b), 1):
        for key in sa:
            assert same_bits(sa[key], sb[key]), (t, key)
        assert ba == bb, t


# ----------------------------------------------------------------------------- against the reference
@pytest.mark.parametrize("name,comm_op", [("distinct_ds_topk", "compress_top_k"), ("exact_ds_sign", "sign")])
def test_deepsqueeze_fused_step_matches_the_reference(name, comm_op):
    fx = golden(f"ef_{name}")
    got, nb = _run_ds(fx, comm_op, _ds_wires(fx, comm_op), "fused_step")
    assert nb.calls == 2
    for t, (snap, bits) in enumerate(got, 1):
        for key in ("params", "mem", "bufs"):
            assert same_bits(snap[key], fx[f"s{t}_{key}"]), (t, key)
        assert same_bits(snap["grad"], fx["g"][t - 1]), "apply mode leaves the gradients as they were set"
        if float(fx["hp"][1]) == 0.0:
            assert same_bits(snap["grad"], fx[f"s{t}_grad"]), (t, "grad")
        assert bits == float(fx[f"s{t}_n_bits"]), t


def test_ef_sign_fused_step_matches_the_reference():
    fx = golden("ef_exact_efsign")
    got, nb = _run_ef(fx, _ef_wires(fx), "fused_step")
    assert nb.calls == 2
    for t, (snap, bits) in enumerate(got, 1):
        for key in ("params", "mem", "bufs", "grad"):
            assert same_bits(snap[key], fx[f"s{t}_{key}"]), (t, key)
        assert bits == float(fx[f"s{t}_n_bits"]), t


@pytest.mark.parametrize("name,comm_op", [("distinct_ds_topk", "compress_top_k"), ("exact_ds_sign", "sign")])
def test_deepsqueeze_step_loop_matches_the_reference(name, comm_op):
    """The yardstick itself: step_loop is the reference's op sequence."""
    fx = golden(f"ef_{name}")
    got, _ = _run_ds(fx, comm_op, _ds_wires(fx, comm_op), "step_loop")
    for t, (snap, bits) in enumerate(got, 1):
        for key in ("params", "mem", "bufs"):
            assert same_bits(snap[key], fx[f"s{t}_{key}"]), (t, key)


def test_ef_sign_step_loop_matches_the_reference():
    fx = golden("ef_exact_efsign")
    got, _ = _run_ef(fx, _ef_wires(fx), "step_loop")
    for t, (snap, bits) in enumerate(got, 1):
        for key in ("params", "mem", "bufs", "grad"):
            assert same_bits(snap[key], fx[f"s{t}_{key}"]), (t, key)


# ----------------------------------------------------------------------------- fused against loop
@pytest.mark.parametrize("comm_op,q", [("quantize_qsgd", 4), ("quantize_qsgd", 32), ("compress_random_k", 4)],
                         ids=["qsgd-q4", "qsgd-q32", "random-k"])
def test_deepsqueeze_fused_step_matches_step_loop(comm_op, q):
    """The compressors whose draws are this codec's own, with the drawn seeds pinned per step."""
    fx = golden("ef_distinct_ds_topk")
    wires = _ds_wires(fx, comm_op, q)
    fused, _ = _run_ds(fx, comm_op, wires, "fused_step", q)
    loop, _ = _run_ds(fx, comm_op, wires, "step_loop", q)
    _assert_same_runs(fused, loop)
    assert not same_bits(fused[1][0]["mem"], fx["mem0"])


@pytest.mark.parametrize("comm_op", ["compress_top_k", "sign"])
def test_deepsqueeze_bf16_model_fused_matches_loop(comm_op):
    fx = golden("ef_distinct_ds_topk")
    wires = _ds_wires(fx, comm_op)
    fused, _ = _run_ds(fx, comm_op, wires, "fused_step", dtype=torch.bfloat16)
    loop, _ = _run_ds(fx, comm_op, wires, "step_loop", dtype=torch.bfloat16)
    _assert_same_runs(fused, loop)


def test_ef_sign_bf16_model_fused_matches_loop():
    fx = golden("ef_exact_efsign")
    wires = _ef_wires(fx)
    fused, _ = _run_ef(fx, wires, "fused_step", dtype=torch.bfloat16)
    loop, _ = _run_ef(fx, wires, "step_loop", dtype=torch.bfloat16)
    _assert_same_runs(fused, loop)


# ----------------------------------------------------------------------------- launches and the CPU path
def _counts():
    from chocosgd_amd import codec
    return {k: codec.launch_count(k) for k in ("param_pack_kernel", "param_unpack_kernel", "param_ef_kernel")}


def test_fused_steps_launch_no_pack_and_no_unpack():
    """10 tensors: one launch per params_ef call; two per DeepSqueeze step, one per EF-sign step."""
    from chocosgd_amd import deep_squeeze, ef_sign
    fx = golden("ef_exact_ds_sign")
    wires = _ds_wires(fx, "sign")
    m, nb = _Model(fx), _Neighbours()
    assert len(m.params) == 10
    comp = deep_squeeze.DeepSqueezeCompressor(aggregator=nb, rank=RANK, **_ds_args("sign", float(fx["gamma"])))
    mem_ptr = m.memory.buffer.data_ptr()
    for t in (1, 2):
        m.set_grads(fx["g"][t - 1])
        nb.msgs = wires[t]
        c0 = _counts()
        deep_squeeze.fused_step(comp, m.groups, m.names, m.state, m.shapes, m.memory, INFO)
        c1 = _counts()
        assert c1["param_pack_kernel"] == c0["param_pack_kernel"]
        assert c1["param_unpack_kernel"] == c0["param_unpack_kernel"]
        assert c1["param_ef_kernel"] - c0["param_ef_kernel"] == 2
    assert m.memory.buffer.data_ptr() == mem_ptr, "the memory is updated in place"
    fx = golden("ef_exact_efsign")
    wires = _ef_wires(fx)
    m, nb = _Model(fx), _Neighbours()
    comp = ef_sign.EFSignCompressor(rank=RANK, world_size=W, aggregator=nb, comm_op="sign", comm_device="gpu",
                                    use_ipc=False)
    mem_ptr = m.memory.buffer.data_ptr()
    for t in (1, 2):
        m.set_grads(fx["g"][t - 1])
        nb.msgs = wires[t]
        c0 = _counts()
        ef_sign.fused_step(comp, m.groups, m.names, m.state, m.memory)
        c1 = _counts()
        assert c1["param_pack_kernel"] == c0["param_pack_kernel"]
        assert c1["param_unpack_kernel"] == c0["param_unpack_kernel"]
        assert c1["param_ef_kernel"] - c0["param_ef_kernel"] == 1
    assert m.memory.buffer.data_ptr() == mem_ptr, "the memory is updated in place"


class _HostCompressor:
    """A compressor of torch ops alone, for a CPU model: the message is the buffer itself, the
    local copy half of it.  It has no `residual` keyword: only step_loop can drive it."""

    world_size = W

    def __init__(self):
        self.calls = []

    def compress(self, arg):
        from chocosgd_amd.tensor_buffer import TensorBuffer
        self.calls.append("compress")
        tb = arg["params_tb"] if isinstance(arg, dict) else arg
        local = TensorBuffer.from_flat(tb.buffer * 0.5, tb._tensors_sizes)
        if isinstance(arg, dict):
            arg["n_bits"] = 17
            return local
        return {"synced_grads_tb": local, "n_bits": 17}

    def sync(self, sb):
        self.calls.append("sync")

    def uncompress(self, sb, neighbors_info):
        from chocosgd_amd.tensor_buffer import TensorBuffer
        tb = sb["params_tb"]
        return TensorBuffer.from_flat(torch.full_like(tb.buffer, 0.25), tb._tensors_sizes)

    def decompress(self, sb):
        return sb["synced_grads_tb"]


def test_a_cpu_model_takes_step_loop():
    from chocosgd_amd import deep_squeeze, ef_sign
    fx = golden("ef_exact_ds_sign")
    c0 = _counts()
    results = []
    for which in ("fused_step", "step_loop"):
        m, comp = _Model(fx, device="cpu"), _HostCompressor()
        m.set_grads(fx["g"][0])
        bits = getattr(deep_squeeze, which)(comp, m.groups, m.names, m.state, m.shapes, m.memory, INFO)
        assert bits == 17 and comp.calls == ["compress", "sync"]
        results.append(m.snapshot())
    for key in results[0]:
        assert same_bits(results[0][key], results[1][key]), key
    # params = (p0 - lr * g) + 0.25, memory = half of (mem0 + p0 - lr * g): exact on this set
    lr = float(fx["hp"][0])
    sgd = fx["p0"] - np.float32(lr) * fx["g"][0]
    assert same_bits(results[0]["params"], sgd + np.float32(0.25))
    assert same_bits(results[0]["mem"], (fx["mem0"] + sgd) * np.float32(0.5))
    fx = golden("ef_exact_efsign")
    results = []
    for which in ("fused_step", "step_loop"):
        m, comp = _Model(fx, device="cpu"), _HostCompressor()
        m.set_grads(fx["g"][0])
        assert getattr(ef_sign, which)(comp, m.groups, m.names, m.state, m.memory) == 17
        results.append(m.snapshot())
    for key in results[0]:
        assert same_bits(results[0][key], results[1][key]), key
    assert _counts() == c0, "a CPU model launches nothing"
