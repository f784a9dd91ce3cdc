"""Consensus evaluation (drop-in for the model-difference half of
dl_code/pcode/utils/auxiliary.py, and what --evaluate_consensus does with it).

The reference, at every evaluation (distributed_running_cv.py:110-115, :239-243): deep-copies the
model, averages the copy over the workers with agg_model(copy, op="avg") -- one all-reduce and one
division per parameter tensor (communication.py:114-122) -- and logs get_model_difference(model,
copy) -- one subtraction per tensor, a concatenation, an fp32 norm and an .item()
(auxiliary.py:18-34).

Here: ONE pack launch per chunk of the parameters into a flat fp32 buffer, ONE collective, and
codec.params_consensus -- one launch per chunk of 128 tensors that divides the sum, takes the
difference to this worker's parameters, accumulates its square in fp64 and (optionally) writes
the averaged model, plus one launch that adds the partial sums in a fixed order.  Without
`avg_out` no copy of the model is ever made.

Differences from the reference, by design:
  * the averaged model is written into the tensors' own storage; `param.data` is never rebound;
  * the sum over the workers is taken on the parameters widened to fp32 (the reference all-reduces
    a 16-bit model in 16 bits);
  * for a 16-bit model the distance is to the unrounded fp32 average (with master=: from the fp32
    master copy); for an fp32 model every element-wise value is the reference's;
  * the norm is accumulated in fp64 and rounded once (the reference's fp32 Tensor.norm() is the
    inaccurate one).
"""
import torch

from . import codec

_TILE = 8192      # flat elements per workgroup (csrc/param_common.h kPbTile)
_WAVE_MAX = 1024  # a span of at most this many elements is summed by one wave (csrc/consensus.hip)


# ----------------------------------------------------------------------------- arguments
def _tensor_list(x, what, grads=False):
    """The tensors of a module's parameters (or their gradients), or of a list."""
    items = list(x.parameters()) if isinstance(x, torch.nn.Module) else list(x)
    if grads:
        items = [p.grad for p in items]  # a parameter without a gradient raises below, as the reference's access would
        if any(g is None for g in items):
            raise AttributeError(f"{what}: a parameter has no gradient")
    for i, t in enumerate(items):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{what}: entry {i} is not a tensor")
    return items


def _master_buffer(master, n):
    if master is None:
        return None
    buf = master.buffer if hasattr(master, "buffer") else master
    if not isinstance(buf, torch.Tensor) or buf.dtype != torch.float32 or buf.dim() != 1 or buf.numel() != n:
        raise RuntimeError(f"master must be (or hold) a flat float32 buffer of {n} elements")
    return buf


def _kernels_take(tensors, *others):
    """Whether the batched kernels take these: contiguous float32 / bfloat16 / float16 tensors on
    one ROCm device (and every flat tensor of `others` contiguous fp32 on it)."""
    if not tensors or not tensors[0].is_cuda:
        return False
    dev = tensors[0].device
    if not all(t.device == dev and t.dtype in codec.PARAM_DTYPES and t.is_contiguous() for t in tensors):
        return False
    return all(o is None or (o.device == dev and o.is_contiguous()) for o in others)


def _matching(avg_out, tensors):
    if avg_out is None:
        return None
    out = _tensor_list(avg_out, "avg_out")
    if len(out) != len(tensors) or any(o.numel() != t.numel() for o, t in zip(out, tensors)):
        raise RuntimeError("avg_out must hold one tensor of the same size for every parameter")
    return out


_plans = []  # the last few parameter lists' plans (tables, workspace, output)


def _plan_for(tensors):
    for plan in _plans:
        if plan.holds(tensors):
            break
    else:
        plan = codec.ParamSgdPlan(tensors)
        _plans.append(plan)
        del _plans[:-4]
    for i, t in enumerate(tensors):
        plan.param_ptrs[i] = t.data_ptr()
    return plan


def _divisor(aggregator, distributed):
    return float(aggregator.world_size) if distributed else 1.0


# ----------------------------------------------------------------------------- the kernels' summation order
def _butterfly(acc):
    """The xor butterfly (32, 16, ..., 1) over the last dimension of 64 lane sums; lane 0's value."""
    lanes = torch.arange(64, device=acc.device)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lanes ^ o]
    return acc[..., 0]


def _span_sum(sq, a):
    """The fp64 sum of `sq`, the squares of flat elements [a, a + len(sq)) of one tensor inside one
    tile, in the order choco_params_consensus adds them (include/choco_codec.h)."""
    m = sq.numel()
    if m <= _WAVE_MAX:
        rows = torch.nn.functional.pad(sq, (0, -m % 64)).view(-1, 64)
        acc = rows[0]
        for r in rows[1:]:
            acc = acc + r
        return _butterfly(acc)
    lead = a & 7  # groups sit at absolute flat offsets
    cells = torch.nn.functional.pad(sq, (lead, -(lead + m) % 2048)).view(-1, 256, 8)
    acc = torch.zeros(256, dtype=sq.dtype, device=sq.device)
    for it in range(cells.shape[0]):
        for k in range(8):
            acc = acc + cells[it, :, k]
    w = _butterfly(acc.view(4, 64))
    return ((w[0] + w[1]) + w[2]) + w[3]


def ordered_sums(values, lens):
    """Per tensor, the fp64 sum of squares of `values` (flat, laid out by `lens`) in the kernels'
    fixed order: per (8192-element tile, tensor) one partial, a tensor's partials in ascending
    tile order.  Returns a list of 0-dim fp64 tensors (a zero-length tensor: 0)."""
    sq = values.double()
    sq = sq * sq
    out, o0 = [], 0
    for m in lens:
        acc = torch.zeros((), dtype=torch.float64, device=values.device)
        a = o0
        while a < o0 + m:
            b = min(o0 + m, (a // _TILE + 1) * _TILE)
            acc = acc + _span_sum(sq[a:b], a)
            a = b
        out.append(acc)
        o0 += m
    return out


def _total(sums, device):
    acc = torch.zeros((), dtype=torch.float64, device=device)
    for s in sums:
        acc = acc + s
    return acc


# ----------------------------------------------------------------------------- consensus evaluation
def consensus_eval_loop(params, aggregator, avg_out=None, master=None, per_tensor=False, distributed=True):
    """consensus_eval as one torch op per line: the pack (widening to fp32 is exact), the sum over
    the workers, a true division by a 0-dim tensor, the subtraction, the fp64 sums of squares in
    the kernels' order (ordered_sums), the square root and one rounding to fp32.  The path CPU
    tensors, other dtypes, non-contiguous tensors and tensors on several devices keep; same bits
    as the kernels."""
    tensors = [t.detach() for t in _tensor_list(params, "params")]
    out = _matching(avg_out, tensors)
    lens = [t.numel() for t in tensors]
    floating = all(t.dtype in codec.PARAM_DTYPES for t in tensors)
    dev = tensors[0].device
    x = torch.cat([(t.float() if floating else t).reshape(-1).to(dev) for t in tensors])
    mbuf = _master_buffer(master, sum(lens))
    if mbuf is not None:
        x = mbuf.detach().to(dev)
    flat = aggregator._agg(x.clone(), op="sum", distributed=distributed)
    a = flat.div(torch.full((), _divisor(aggregator, distributed), dtype=flat.dtype, device=flat.device))
    d = a - x
    ssd, ssa = ordered_sums(d, lens), ordered_sums(a, lens)
    stats = torch.stack([_total(ssd, dev).sqrt(), _total(ssa, dev).sqrt()]).float()
    if out is not None:
        for o, piece in zip(out, a.split(lens)):
            o.detach().copy_(piece.view(o.shape))  # a converting copy: round to nearest even
    dists = torch.stack(ssd).sqrt().float() if per_tensor else None
    return stats, dists


def consensus_eval(params, aggregator, avg_out=None, master=None, per_tensor=False, distributed=True):
    """The consensus distance of --evaluate_consensus in one pass: the model averaged over the
    workers and this worker's L2 distance to it.

        one pack launch per chunk of the parameters into a flat fp32 buffer (master=: a copy of
            the master buffer instead);
        aggregator._agg(flat, op="sum", distributed=distributed), ONE collective;
        codec.ParamSgdPlan.consensus with divisor = aggregator.world_size (1.0 when not
            distributed; a true division).

    params: a module or a list of tensors.  avg_out: a list of tensors, or a module whose
    parameters match in size, that receives the averaged model narrowed to each tensor's dtype;
    it may be the model itself (the distance is then that of the values from before the call).
    With avg_out=None no copy of the model is ever made.  master: a MasterWeights of this model
    (or its flat fp32 buffer): the sum and the distance are taken on the master values.

    Returns (stats, dists): stats the two-element fp32 device tensor [distance to the average,
    norm of the average] -- the plan's own, overwritten by the next call on the same parameters;
    dists the per-tensor distances (per_tensor) or None.  Nothing is read on the host.  The
    distance is this worker's; for the world's mean all-reduce stats[0] ** 2 yourself.

    Only _agg(op="sum") and .world_size of the aggregator are used: this package's
    CentralizedAggregation and the reference's both serve.  Tensors the kernels do not take run
    consensus_eval_loop.  The differences from the reference are listed in the module docstring."""
    tensors = _tensor_list(params, "params")
    out = _matching(avg_out, tensors)
    n = sum(t.numel() for t in tensors)
    mbuf = _master_buffer(master, n)
    if not _kernels_take(tensors, mbuf) or (out is not None and not (
            _kernels_take(out) and all(o.dtype == t.dtype and o.device == t.device for o, t in zip(out, tensors)))):
        return consensus_eval_loop(params, aggregator, avg_out, master, per_tensor, distributed)
    plan = _plan_for(tensors)
    if mbuf is None:
        flat = torch.empty(n, dtype=torch.float32, device=plan.device)
        codec.params_pack(tensors, flat)
    else:
        flat = mbuf.detach().clone()
    flat = aggregator._agg(flat, op="sum", distributed=distributed)
    dists = torch.empty(plan.nseg, dtype=torch.float32, device=plan.device) if per_tensor else None
    stats = plan.consensus(flat, _divisor(aggregator, distributed), avg_out=out, master=mbuf, dists=dists)
    return stats, dists


class _Identity:
    """The aggregator of get_model_difference: the `sum` is model2 itself."""
    world_size = 1.0

    def _agg(self, data, op=None, distributed=True):
        return data


def get_model_difference(model1, model2):
    """||model2 - model1||_2 over all parameters as a Python float (auxiliary.py:18-34): model2 is
    packed, and the consensus kernel runs on model1 with divisor 1 (an exact division): two
    launches per chunk and one total launch.  The norm is accumulated in fp64 and rounded once
    (the reference takes an fp32 norm); for 16-bit models the difference is the fp32 difference
    of the widened values.  Tensors the kernels do not take go one torch op per line."""
    t1, t2 = _tensor_list(model1, "model1"), _tensor_list(model2, "model2")
    if len(t1) != len(t2) or any(a.numel() != b.numel() for a, b in zip(t1, t2)):
        raise RuntimeError("get_model_difference: the models' parameters do not match in size")
    if _kernels_take(t1) and _kernels_take(t2) and t1[0].device == t2[0].device:
        plan = _plan_for(t1)
        flat = torch.empty(plan.n, dtype=torch.float32, device=plan.device)
        codec.params_pack(t2, flat)
        return plan.consensus(flat, 1.0)[0].item()
    lens = [t.numel() for t in t1]
    dev = t1[0].device
    pack = lambda ts: torch.cat([(t.detach().float() if t.dtype in codec.PARAM_DTYPES else t.detach())  # noqa: E731
                                 .reshape(-1).to(dev) for t in ts])
    a = pack(t2)
    a = a.div(torch.full((), 1.0, dtype=a.dtype, device=dev))
    return _total(ordered_sums(a - pack(t1), lens), dev).sqrt().float().item()


# ----------------------------------------------------------------------------- agg_model / agg_grad
def agg_tensors(aggregator, tensors, op):
    """What CentralizedAggregation.agg_model / agg_grad do with a list of tensors: one pack, one
    all-reduce and one launch per chunk (codec.params_consensus, WRITE_AVG alone) that writes
    sum / world_size ("avg") or the sum ("sum": divisor 1) into the tensors' own storage,
    narrowed once to each tensor's dtype.  float32 / bfloat16 / float16 tensors the kernels do
    not take (CPU, non-contiguous, several devices) follow the same lines one torch op each;
    tensors of other dtypes go per tensor through _agg, as the reference's do."""
    if op not in ("avg", "sum"):
        raise NotImplementedError("op {} is not supported yet.".format(op))
    tensors = list(tensors)
    if not tensors:
        return
    divisor = float(aggregator.world_size) if op == "avg" else 1.0
    if _kernels_take(tensors):
        plan = _plan_for(tensors)
        flat = torch.empty(plan.n, dtype=torch.float32, device=plan.device)
        codec.params_pack(tensors, flat)
        flat = aggregator._agg(flat, op="sum")
        plan.consensus(flat, divisor, avg_out=tensors, want_dist=False)
        return
    tensors = [t.detach() for t in tensors]
    if all(t.dtype in codec.PARAM_DTYPES for t in tensors):
        dev = tensors[0].device
        flat = aggregator._agg(torch.cat([t.float().reshape(-1).to(dev) for t in tensors]), op="sum")
        a = flat.div(torch.full((), divisor, dtype=flat.dtype, device=flat.device))
        for t, piece in zip(tensors, a.split([t.numel() for t in tensors])):
            t.copy_(piece.view(t.shape))
        return
    for t in tensors:
        out = aggregator._agg(t, op=op)
        if out is not t:
            t.copy_(out)
