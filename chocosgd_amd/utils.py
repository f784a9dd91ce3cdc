"""Optimizer-step helpers: drop-in for dl_code/pcode/optim/utils.py (apply_gradient and the
CHOCO half)."""
import torch

from . import codec
from .sparsification import get_n_bits
from .tensor_buffer import TensorBuffer, flatten


def _get_data(param_groups, idx, is_get_grad):
    if is_get_grad:
        return param_groups[idx]["params"][0].grad
    return param_groups[idx]["params"][0]


def apply_gradient_loop(param_groups, state, apply_grad_to_model=True):
    """apply_gradient as one torch op per line and tensor (optim/utils.py:13-47): the path CPU
    tensors, and anything the batched kernel does not take, keep.  Same results as the
    reference, with the two differences apply_gradient documents."""
    for group in param_groups:
        weight_decay, momentum = group["weight_decay"], group["momentum"]
        dampening, nesterov = group["dampening"], group["nesterov"]
        for p in group["params"]:
            if p.grad is None:
                continue
            d_p = p.grad.data
            if weight_decay != 0:
                d_p = d_p.add(p.data, alpha=weight_decay)  # out of place: p.grad keeps its values
            if momentum != 0:
                param_state = state[p]
                if "momentum_buffer" not in param_state:
                    buf = param_state["momentum_buffer"] = torch.zeros_like(p.data)
                    buf.mul_(momentum).add_(d_p)
                else:
                    buf = param_state["momentum_buffer"]
                    buf.mul_(momentum).add_(d_p, alpha=1 - dampening)
                d_p = d_p.add(buf, alpha=momentum) if nesterov else buf
            if apply_grad_to_model:
                p.data.add_(d_p, alpha=-group["lr"])
            else:
                p.grad.data.copy_(d_p)  # into the grad's own storage: p.grad is not rebound


_plans = {}  # id of a list's first parameter -> its ParamSgdPlan (which holds weak references only)


def _sgd_plan(params):
    """The cached plan of this parameter list, or None where the batched kernel does not take
    it (CPU tensors, other dtypes, non-contiguous or several devices)."""
    plan = _plans.get(id(params[0]))
    if plan is not None and plan.holds(params):
        return plan
    dev = params[0].device
    if not all(p.is_cuda and p.device == dev and p.dtype in codec.PARAM_DTYPES and p.is_contiguous()
               for p in params):
        return None
    if len(_plans) >= 64:  # plans of parameter lists long gone
        _plans.clear()
    plan = _plans[id(params[0])] = codec.ParamSgdPlan(params)
    return plan


def _sgd_batched(entries, state, apply_grad_to_model, flat, write):
    """One batched launch (per chunk) for `entries`, a list of (group, param) in flat order.
    Returns False, with nothing changed, where a tensor cannot take it."""
    plan = _sgd_fill(entries, state, apply_grad_to_model, flat)
    if plan is None:
        return False
    plan.run(flat, grad_mode=not apply_grad_to_model, write=write)
    return True


def _sgd_fill(entries, state, apply_grad_to_model, flat):
    """The plan of `entries` with this step's pointers, flags and hyperparameters written (and
    missing momentum buffers created), ready to run; None, with nothing changed, where a tensor
    cannot take the batched kernels."""
    if not entries:
        return None
    params = [p for _, p in entries]
    plan = _sgd_plan(params)
    if plan is None or (flat is not None and (flat.dtype != torch.float32 or flat.device != plan.device
                                              or flat.numel() != plan.n or not flat.is_contiguous())):
        return None
    pp, gp, bp, flags, seen = plan.param_ptrs, plan.grad_ptrs, plan.buf_ptrs, plan.flags, plan.seen
    created = []
    ok = True
    for i, (group, p) in enumerate(entries):
        momentum = group["momentum"]
        g = p.grad
        if g is None:
            if not apply_grad_to_model:  # the reference skips it; a flat gradient has no slot to skip
                ok = False
                break
            pp[i], gp[i], bp[i], flags[i] = p.data_ptr(), None, None, codec.SGD_F_NOGRAD
            continue
        fl = codec.SGD_F_NESTEROV if group["nesterov"] else 0
        b_ptr = None
        if momentum != 0:
            param_state = state[p]
            buf = param_state.get("momentum_buffer")
            if buf is None:  # written, not read, by its first step
                buf = param_state["momentum_buffer"] = torch.zeros_like(p.data)
                created.append(param_state)
                fl |= codec.SGD_F_FIRST
            if not plan.fits(i, buf):
                ok = False
                break
            b_ptr = buf.data_ptr()
        if not plan.fits(i, g):
            ok = False
            break
        pp[i], gp[i], bp[i], flags[i] = p.data_ptr(), g.data_ptr(), b_ptr, fl
        hp = (group["lr"], group["weight_decay"], momentum, group["dampening"])
        if hp != seen[i]:
            plan.lr[i], plan.weight_decay[i], plan.momentum[i], plan.dampening[i] = hp
            seen[i] = hp
    if not ok:
        for param_state in created:
            del param_state["momentum_buffer"]
        return None
    return plan


def apply_gradient(param_groups, state, apply_grad_to_model=True, flat_out=None):
    """optim/utils.py:13-47: weight decay, momentum with dampening, optional Nesterov, then
    p -= lr * d_p (apply_grad_to_model) or d_p left as the gradient.  Missing
    state[p]["momentum_buffer"] entries are created.  fp32 / bf16 / fp16 ROCm tensors take ONE
    batched HIP launch per chunk of tensors (codec.params_sgd); CPU tensors, and anything else,
    the per-tensor loop above.

    flat_out (a TensorBuffer or a flat fp32 tensor over every parameter, in group order): it
    receives, in the same pass, the new parameters (what recover_params' flatten would build
    next) or, with apply_grad_to_model=False, d_p (what get_data(is_get_grad=True) +
    TensorBuffer would).

    Two differences from the reference, by design: with apply_grad_to_model the grad tensors
    are never written (the reference adds the weight decay into p.grad in place); without it
    d_p is written into the existing grad tensors' storage and p.grad is not rebound to the
    momentum buffer object."""
    entries = [(group, p) for group in param_groups for p in group["params"]]
    flat = getattr(flat_out, "buffer", flat_out)
    if _sgd_batched(entries, state, apply_grad_to_model, flat, write=True):
        return
    apply_gradient_loop(param_groups, state, apply_grad_to_model)
    if flat is not None:
        flat.copy_(flatten([p.data if apply_grad_to_model else p.grad.data for _, p in entries], dtype=flat.dtype))


def recover_params(param_groups, param_names, rank=None, neighbor_hat_params=None, get_hat_params=True):
    """optim/utils.py:50-64: flat copies of the params (and of x_hat_i).

    The flat buffers of an fp32 / bf16 / fp16 model are fp32, as the reference's are
    (communication.py:69-75 widens any model into the default dtype): the gossip step, the
    delta and the message are computed from the unrounded fp32 copy, and only unpack() rounds
    back to the model's precision (tensor_buffer.py:38-40)."""
    params = [_get_data(param_groups, idx, False) for idx, _ in param_names]
    params = [p for p in params if p is not None]
    floating = all(p.dtype in codec.PARAM_DTYPES for p in params)
    flatten_params = TensorBuffer(params, dtype=torch.float32 if floating else None)
    if get_hat_params:
        assert neighbor_hat_params is not None and rank is not None
        hat = torch.empty_like(flatten_params.buffer)
        hat.copy_(neighbor_hat_params[rank].buffer)
        flatten_hat_params = TensorBuffer.from_flat(hat, [p.size() for p in params])
        return params, flatten_params, flatten_hat_params
    return params, flatten_params


def fused_step(compressor, param_groups, param_names, shapes, neighbor_hat_params, neighbors_info,
               consensus_stepsize, rank, defer_receive=False, state=None):
    """ParallelCHOCO_V.step after apply_gradient (parallel_choco_v.py:115-155), with the
    consensus step fused into the compressor's first pass: recover_params, then
    compress (x += gamma * (memory - x_hat_i) and d = x_new - x_hat_i in one pass), sync,
    uncompress, and the updated x unpacked into the model.  Returns the sync_buffer.
    The reference runs update_params_from_neighbor as its own pass before compress.

    defer_receive=True (QSGD, sign): this step's uncompress is applied by the NEXT step's
    compress, in the same pass as that step's consensus step (the reference's step runs
    the previous step's join, then update_params_from_neighbor, with only apply_gradient
    -- which touches x alone -- in between, parallel_choco_v.py:104-131).  x is the same
    after every step; x_hat / memory lag by one step until the next step or
    compressor.flush_receive() (call it before reading or saving them).  flatten_hat_params
    is x_hat_i itself, not a copy (the pass updates it in place).

    state (optimizer.state; default None: the caller has run apply_gradient, as above): the
    step runs apply_gradient itself, as the fused SGD + pack launch -- one pass that reads p,
    g and the momentum buffer and writes the buffer and the flat x.  The launch does not write
    the params (the unpack at the end writes them and nothing in between reads them) and
    recover_params' pack is skipped.  Every group must hold one parameter, named in
    param_names, as the reference's groups do."""
    flatten_params = None
    if state is not None:
        flatten_params = _sgd_packed(param_groups, param_names, state)
    if defer_receive:
        if flatten_params is None:
            params, flatten_params = recover_params(param_groups, param_names, get_hat_params=False)
        else:
            params = [_get_data(param_groups, idx, False) for idx, _ in param_names]
        flatten_hat_params = neighbor_hat_params[rank]
    else:
        if hasattr(compressor, "flush_receive"):  # a receive an earlier deferred step left
            compressor.flush_receive()
        if flatten_params is None:
            params, flatten_params, flatten_hat_params = recover_params(param_groups, param_names, rank,
                                                                        neighbor_hat_params, get_hat_params=True)
        else:
            params = [_get_data(param_groups, idx, False) for idx, _ in param_names]
            hat = torch.empty_like(flatten_params.buffer)
            hat.copy_(neighbor_hat_params[rank].buffer)
            flatten_hat_params = TensorBuffer.from_flat(hat, [p.size() for p in params])
    sync_buffer = {"original_shapes": shapes, "flatten_params": flatten_params,
                   "flatten_hat_params": flatten_hat_params,
                   "gossip": (neighbor_hat_params["memory"].buffer, consensus_stepsize)}
    if defer_receive:
        sync_buffer["defer_receive"] = True
    compressor.pipeline(sync_buffer, neighbor_hat_params, neighbors_info)
    flatten_params.unpack(params)
    return sync_buffer


def _sgd_packed(param_groups, param_names, state):
    """fused_step(state=...): apply_gradient and the pack of the new params in one launch.
    Returns the flat TensorBuffer, or None after the per-tensor loop has updated the params
    (tensors the batched kernel does not take: recover_params packs them as before)."""
    entries = step_entries(param_groups, param_names, "fused_step(state=...)")
    dev = entries[0][1].device
    flat = torch.empty(sum(p.numel() for _, p in entries), dtype=torch.float32, device=dev)
    if dev.type == "cuda" and _sgd_batched(entries, state, True, flat, write=False):
        return TensorBuffer.from_flat(flat, [p.size() for _, p in entries])
    apply_gradient_loop(param_groups, state, True)
    return None


def step_entries(param_groups, param_names, what, need_grads=False):
    """[(group, param)] in param_names' order for a step that runs apply_gradient itself: every
    group must hold one parameter, named once in param_names, as the reference's groups do.
    need_grads: a parameter without a gradient raises (the flat gradient buffer the reference
    builds with get_data(is_get_grad=True) has no slot for it)."""
    if len(param_names) != len(param_groups) or any(len(g["params"]) != 1 for g in param_groups) \
            or sorted(idx for idx, _ in param_names) != list(range(len(param_groups))):
        raise RuntimeError(f"{what} needs one parameter per group, each named once in param_names")
    entries = [(param_groups[idx], param_groups[idx]["params"][0]) for idx, _ in param_names]
    if need_grads:
        for idx, name in param_names:
            if param_groups[idx]["params"][0].grad is None:
                raise RuntimeError(f"{what}: parameter {name!r} has no gradient")
    return entries


def mix_sources(buffers, n, device):
    """Whether codec.params_mix takes `buffers` (flat tensors) as its sources for a layout of n
    elements on `device`."""
    return (device.type == "cuda" and 1 <= len(buffers) <= 64
            and all(b.is_cuda and b.device == device and b.dtype == torch.float32 and b.numel() == n
                    and b.is_contiguous() for b in buffers))


def grad_step_plan(entries, state, neighbor_hat_params):
    """The first line of DCD_PSGD.step / ECD_PSGD.step, apply_gradient(apply_grad_to_model=False),
    as the batched launch where the mix kernel can follow it: returns the plan whose tables the
    mix reuses, or None, with nothing changed, where the kernels do not take the tensors (CPU
    tensors, other dtypes, replicas that are not flat fp32 buffers of the model's size)."""
    params = [p for _, p in entries]
    hats = [h.buffer for h in neighbor_hat_params.values()]
    if not mix_sources(hats, sum(p.numel() for p in params), params[0].device):
        return None
    plan = _sgd_fill(entries, state, False, None)
    if plan is not None:
        plan.run(None, grad_mode=True, write=True)
    return plan


def weighted_sum(buffers, weights):
    """sum([b * w for ...]): the reference's own expression, one torch op per term."""
    return sum([b * w for b, w in zip(buffers, weights)])


def dpsgd_step_loop(param_groups, param_names, state, aggregator):
    """dpsgd_step as the reference's op sequence (sgd.py:94-121), one torch op per line: the path
    CPU tensors, and anything the batched kernels do not take, keep."""
    apply_gradient_loop(param_groups, state, True)
    params, flatten_params = recover_params(param_groups, param_names, get_hat_params=False)
    flatten_params.buffer = aggregator._agg(flatten_params.buffer, op="weighted")
    flatten_params.unpack(params)
    return get_n_bits(flatten_params.buffer)


def dpsgd_step(param_groups, param_names, state, aggregator, neighbors_info):
    """The decentralized branch of SGD.step (sgd.py:94-121), plain D-PSGD: apply_gradient fused
    with the pack of the new params (one launch; the params themselves are not written yet),
    the exchange of the flat fp32 buffer (_agg(op="get_raw_sync_data")), and ONE mix launch
    that writes sum(x_r * w_r) straight into the params (communication.py:271-277 and the
    unpack of sgd.py:118).  Returns n_bits.  Tensors the kernels do not take run
    dpsgd_step_loop."""
    entries = step_entries(param_groups, param_names, "dpsgd_step")
    params = [p for _, p in entries]
    dev = params[0].device
    flat = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=dev)
    plan = _sgd_fill(entries, state, True, flat)
    if plan is None:
        return dpsgd_step_loop(param_groups, param_names, state, aggregator)
    plan.run(flat, grad_mode=False, write=False)
    local_data = aggregator._agg(flat, op="get_raw_sync_data")
    srcs = list(local_data.values())
    weights = [neighbors_info[r] for r in local_data]
    # the running sum of more than one launch's sources needs a flat buffer of its own
    run = torch.empty_like(flat) if len(srcs) > 8 else None
    plan.mix(srcs, weights, mode=codec.MIX_WRITE_PARAMS, flat_out=run)
    return get_n_bits(flat)


def update_params_from_neighbor(neighbor_hat_params, flatten_params, consensus_stepsize, self_rank):
    """optim/utils.py:67-72:  x += gamma * (memory - x_hat_i), one fused HIP pass."""
    codec.gossip_step(flatten_params.buffer, neighbor_hat_params["memory"].buffer,
                      neighbor_hat_params[self_rank].buffer, consensus_stepsize)
