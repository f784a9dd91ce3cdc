"""The communication half of DGC (dl_code/pcode/optim/dgc.py:153-252, with
compress_or_quantize at :327-343): error-feedback top-k / random-k of every
gradient tensor, an all-gather of the [values | indices] messages and the
averaged sparse update -- or, for a quantize op, the QSGD dense floats all-reduced.

`DGCCodec(world_aggregator, comm_op, comm_device, n_nodes, quantize_level=, is_biased=,
strict_reference=True)` keeps the reference's three steps as methods:
  * `compress(grads, memory_tb, compress_ratio)` -> (values, indices, n_bits):
    _grad = grad + memory per tensor, top-k of _grad, memory <- `_grad * nmask`
    (dgc.py:174-176).  The reference's nmask is `(~mask.byte()).float()`
    (sparsification.py:33-38): a bitwise NOT of uint8 under the PyTorch this
    runs on, i.e. 255 for unselected and 254 for selected entries, and
    `strict_reference=True` (the default) reproduces exactly that, bit for bit.
    `strict_reference=False` applies the evident intent instead (1 - mask, what `~`
    gave for a ByteTensor in PyTorch <= 1.1: the selected entries zeroed, the rest
    kept).  The error-feedback memory is ONE flat TensorBuffer (the reference keeps a
    dict of per-parameter vectors) so the whole layout is one batched launch;
    `indices` are GLOBAL int32.  For a quantize op the reference leaves memory alone
    (dgc.py:183-185): _grad = grad + memory is a temporary;
  * `sync(values, indices)` -> (synced_message, message_size);
  * `recover_info(flatten_params, synced_message, message_size, lr)` -> params - lr *
    (sum of messages) / n_nodes.
The momentum-factor masking of dgc.py:175-179 (`mask_momentum`) is optimizer state:
`compress(..., momentum_buffers=[...])` applies it (strict_reference=False only) in the same
batched launch that clears the selected memory; without that argument it is not applied, and
`last_indices` holds the selected global indices.

The optimizer half (dgc.py:254-324) is `apply_gradient` below -- DGC._apply_gradient with its
per-tensor gradient clipping, as at most two batched passes -- and `fused_step` is DGC.step
(dgc.py:118-151) end to end.

strict_reference=True multiplies the unselected memory by 255 every step, so the memory
overflows to inf after ~16 steps and DGC top-k / random-k diverges -- as the reference
does on the PyTorch it runs on; a one-time warning says so.
"""
import math
import warnings

import torch

from . import codec, utils
from .communication import recover_device
from .sparsification import _draw_seed, get_n_bits
from .tensor_buffer import flatten
from .wire import _Layout, _received, _staged


_warned = []


def _warn_strict_once():
    if not _warned:
        _warned.append(True)
        warnings.warn("DGCCodec(strict_reference=True) reproduces the reference's nmask = "
                      "(~mask.byte()).float() = 255 / 254 (sparsification.py:33-38): the error-feedback "
                      "memory grows 255x per step and overflows after ~16 steps; pass "
                      "strict_reference=False for the intended 1 - mask", RuntimeWarning, stacklevel=3)


class DGCCodec(object):
    def __init__(self, world_aggregator, comm_op, comm_device, n_nodes, quantize_level=None, is_biased=False,
                 strict_reference=True):
        self.strict_reference = strict_reference
        self.world_aggregator = world_aggregator
        self.comm_op = comm_op
        self.comm_device = comm_device
        self.n_nodes = n_nodes
        self.quantize_level = quantize_level
        self.is_biased = is_biased
        self.is_compress_op = "compress" in comm_op
        self.selected_shapes = None
        self.last_indices = None
        if strict_reference and "compress" in comm_op:
            _warn_strict_once()

    def compress(self, grads, memory_tb, compress_ratio, momentum_buffers=None, grads_in_memory=False):
        """grads_in_memory: the caller's SGD launch has already added d_p into the memory
        (apply_gradient(flat_out=memory_tb, add_flat=True)), so flatten + add_ are skipped.
        momentum_buffers (one per tensor, None entries allowed): the momentum-factor masking of
        dgc.py:178-182, in the launch that also clears the selected memory (the same bits as
        the separate clear leaves)."""
        if momentum_buffers is not None:
            if self.strict_reference:
                # the reference's nmask multiplies the buffers by 255 / 254 every step
                raise RuntimeError("momentum_buffers needs strict_reference=False: the reference's 255 / 254 "
                                   "mask would multiply the momentum buffers by 255 per step")
            if not self.is_compress_op:
                raise RuntimeError("momentum-factor masking belongs to the compress ops (dgc.py:174-182)")
            if len(momentum_buffers) != len(grads):
                raise RuntimeError("momentum_buffers needs one entry (or None) per gradient")
        if grads_in_memory and not self.is_compress_op:
            raise RuntimeError("a quantize op leaves the memory alone (dgc.py:183-185): grads_in_memory is "
                               "for the compress ops")
        memory = memory_tb.buffer
        lens = tuple(int(g.nelement()) for g in grads)
        lay = _Layout.get(lens, memory.device)
        if self.is_compress_op:
            x = memory
            if not grads_in_memory:
                x.add_(flatten(grads))  # _grad = grad + memory (dgc.py:157; fp32 add commutes), in place
            plan = lay.topk_plan(float(compress_ratio))
            if "top_k" in self.comm_op:
                values, indices = codec.topk_segmented(x, plan)
            elif "random_k" in self.comm_op:
                values, indices = codec.randk_segmented(x, plan, _draw_seed(), is_biased=True)
            else:
                raise NotImplementedError
            if self.strict_reference:
                # _grad * nmask with nmask = (~mask.byte()).float(): 255 unselected, 254 selected
                x.mul_(255.0)
                x.index_put_((indices.long(),), values * 254.0)
            elif momentum_buffers is not None:
                # buf.mul_(1 - mask) and _grad * (1 - mask) at the selected positions, one launch
                codec.params_mask(momentum_buffers, values, indices, plan.k_per_seg, memory=x, lens=lens,
                                  dtypes=[g.dtype for g in grads])
            else:
                # _grad * (1 - mask): the selected entries (values == x[idx]) become 0
                codec.sparse_accumulate(torch.neg(values), indices, x, 1.0)
            self.selected_shapes = list(plan.k_per_seg)
            self.last_indices = indices
            # nominal bits as compress_or_quantize counts them (dgc.py:335-337): fp32 values and
            # the int64 indices torch.topk returns (the wire here carries int32)
            return values, indices, 32 * values.numel() + 64 * indices.numel()
        if "quantize" in self.comm_op:
            x = memory + flatten(grads)  # _grad: a temporary, memory keeps its value (dgc.py:183-185)
            q = int(self.quantize_level)
            if q == 32:
                dense = x.clone()
            else:
                _, _, dense = codec.qsgd_compress(x, q, is_biased=self.is_biased, seg_off=lay.seg_off, nseg=lay.nseg,
                                                  seed=_draw_seed(), want_dense=True)
            self.selected_shapes = list(lens)
            return dense, None, get_n_bits(dense) * q / 32
        raise NotImplementedError

    def sync(self, selected_values, selected_indices):
        if self.is_compress_op:
            # the sparse wire [values | indices] (codec.sparse_wire), joined here: this method takes
            # the two tensors compress returned, and they need not share one buffer
            message = _staged(torch.cat([selected_values.view(torch.int32), selected_indices]), self.comm_device)
            synced = self.world_aggregator._agg(message, communication_scheme="all_gather")
        else:
            message = _staged(selected_values, self.comm_device)
            synced = self.world_aggregator._agg(message, op="sum", communication_scheme="all_reduce")
        return synced, len(message)

    def recover_info(self, flatten_params, synced_message, message_size, lr):
        if self.is_compress_op:
            grads = torch.zeros_like(flatten_params)
            ranks = ((rank, grads) for rank in range(len(synced_message)))
            for _, _, (values, indices) in _received(synced_message, ranks, codec.sparse_split, message_size):
                # empty_grads[q_indices] += q_values  (dgc.py:234-242), messages in rank order
                codec.sparse_accumulate(values, indices, grads, 1.0)
            update = grads
        else:
            update = recover_device(synced_message, device=flatten_params.device)
        # true division by n_nodes (a device 0-dim divisor: torch turns a CPU-scalar division
        # into a reciprocal multiply on the GPU), then params.add(-lr, update) (dgc.py:244-249)
        update = update / torch.full((), float(self.n_nodes), dtype=torch.float32, device=flatten_params.device)
        return flatten_params.add(update, alpha=-lr)


# ----------------------------------------------------------------------------- the optimizer half
def _clip_threshold(clip_grad, clip_grad_val, n_nodes):
    """dgc.py:258-262, in double as the reference computes it; None: no clipping."""
    if not clip_grad or clip_grad_val is None:
        return None
    return clip_grad_val * (1.0 / math.sqrt(n_nodes))


def _check_groups(param_groups):
    for group in param_groups:
        if group["momentum"] < 0:
            # DGC builds the first buffer as zeros.add_(d_p), apply_gradient as
            # zeros.mul_(momentum).add_(d_p): the same for momentum >= 0 only
            raise RuntimeError("dgc.apply_gradient needs momentum >= 0")


def apply_gradient_loop(param_groups, state, clip_grad=False, clip_grad_val=None, n_nodes=1, flat_out=None,
                        add_flat=False, norms=None):
    """DGC._apply_gradient (dgc.py:279-324) as one torch op per line and tensor: the path CPU
    tensors, and anything the batched kernels do not take, keep.  Arguments and result as
    apply_gradient below."""
    _check_groups(param_groups)
    thr = _clip_threshold(clip_grad, clip_grad_val, n_nodes)
    entries = [(group, p) for group in param_groups for p in group["params"]]
    flat = getattr(flat_out, "buffer", flat_out)
    if add_flat and flat is None:
        raise RuntimeError("add_flat needs a flat_out")
    used = []
    for i, (group, p) in enumerate(entries):
        weight_decay, momentum = group["weight_decay"], group["momentum"]
        if p.grad is None:
            used.append(None)
            continue
        d_p = p.grad.data
        if weight_decay != 0:
            d_p = d_p.add(p.data, alpha=weight_decay)
        if thr is not None:
            norm = d_p.norm(p=2) if norms is None else norms[i].to(device=d_p.device, dtype=d_p.dtype)
            used.append(norm)
            if d_p.dtype == torch.float32:
                if norm >= thr:
                    d_p = thr / norm * d_p
            elif norm.float() >= thr:
                # a 16-bit tensor: the coefficient stays fp32 and the product is narrowed once, as the
                # batched kernel does (torch would round the 0-dim coefficient to the tensor's dtype)
                d_p = (thr / norm.float() * d_p.float()).to(d_p.dtype)
        if momentum != 0:
            param_state = state[p]
            if "momentum_buffer" not in param_state:
                buf = param_state["momentum_buffer"] = torch.zeros_like(p.data)
                buf.mul_(momentum).add_(d_p)
            else:
                buf = param_state["momentum_buffer"]
                buf.mul_(momentum).add_(d_p, alpha=1 - group["dampening"])
            d_p = d_p.add(buf, alpha=momentum) if group["nesterov"] else buf
        p.grad.data.copy_(d_p)  # into the grad's own storage: p.grad is not rebound
    if flat is not None:
        d = flatten([p.grad.data for _, p in entries], dtype=flat.dtype)
        if add_flat:
            flat.add_(d)
        else:
            flat.copy_(d)
    if thr is None or not entries:
        return None
    dev = entries[0][1].device
    return torch.stack([torch.zeros((), device=dev) if v is None else v.detach().float() for v in used])


def apply_gradient(param_groups, state, clip_grad=False, clip_grad_val=None, n_nodes=1, flat_out=None, add_flat=False,
                   norms=None):
    """DGC._apply_gradient (dgc.py:279-324): weight decay, then -- with clip_grad and a
    clip_grad_val -- each tensor's d_p scaled by threshold / ||d_p|| where its norm reaches
    threshold = clip_grad_val / sqrt(n_nodes) (_clip_gradient, :254-265), then momentum with
    dampening and optional Nesterov; d_p is left as the gradient.  fp32 / bf16 / fp16 ROCm
    tensors take at most two batched passes: codec.params_sqnorm (one launch per chunk of
    tensors and a finish launch; skipped without clipping) and the clipped update (one launch
    per chunk); CPU tensors, and anything else, apply_gradient_loop.

    flat_out (a TensorBuffer or a flat fp32 tensor over every parameter, in group order)
    receives d_p in the same pass; add_flat: flat_out += d_p instead -- `_grad = grad + memory`
    (dgc.py:157) with the error-feedback memory as flat_out.
    norms (an fp32 tensor, one entry per parameter): used in place of the computed norms.
    Returns the norms tensor it used, or None without clipping.

    As utils.apply_gradient, d_p is written into the existing grad tensors' storage and p.grad
    is not rebound to the momentum buffer.  A negative momentum is refused.  The batched norm
    accumulates in fp64, torch's in the gradient's precision."""
    _check_groups(param_groups)
    thr = _clip_threshold(clip_grad, clip_grad_val, n_nodes)
    entries = [(group, p) for group in param_groups for p in group["params"]]
    flat = getattr(flat_out, "buffer", flat_out)
    if add_flat and flat is None:
        raise RuntimeError("add_flat needs a flat_out")
    plan = utils._sgd_fill(entries, state, False, flat) if entries and entries[0][1].is_cuda else None
    if plan is None:
        return apply_gradient_loop(param_groups, state, clip_grad, clip_grad_val, n_nodes, flat_out, add_flat, norms)
    used = None
    if thr is not None:
        used = plan.sqnorm() if norms is None else norms.to(device=plan.device, dtype=torch.float32).contiguous()
    plan.run(flat, grad_mode=True, write=True, norms=used, clip_threshold=thr, add_flat=add_flat)
    return used


def fused_step(codec_, param_groups, param_names, state, memory_tb, compress_ratio, clip_grad=False,
               clip_grad_val=None, mask_momentum=False, rounding=None):
    """DGC.step (dgc.py:118-151) end to end with a DGCCodec: the norms, the clipped update adding
    d_p into the error-feedback memory in the same pass, compress, the momentum-factor masking
    fused with the memory clear, sync, recover_info and the unpack into the model.  Returns
    n_bits.  Every group must hold one parameter, named in order in param_names, as the
    reference's groups do.  A quantize op keeps its memory (dgc.py:183-185) and takes the
    unfused compress."""
    utils.no_rounding("dgc.fused_step", rounding)  # stochastic rounding: not part of this step
    if len(param_names) != len(param_groups) or any(len(g["params"]) != 1 for g in param_groups) \
            or [idx for idx, _ in param_names] != list(range(len(param_groups))):
        raise RuntimeError("dgc.fused_step needs one parameter per group, named in order in param_names")
    if mask_momentum and codec_.is_compress_op and codec_.strict_reference:
        # refused before anything is stepped (compress would refuse it after the update)
        raise RuntimeError("mask_momentum needs DGCCodec(strict_reference=False): the reference's 255 / 254 mask "
                           "would multiply the momentum buffers by 255 per step")
    params = [group["params"][0] for group in param_groups]
    if codec_.is_compress_op:
        apply_gradient(param_groups, state, clip_grad, clip_grad_val, codec_.n_nodes, flat_out=memory_tb,
                       add_flat=True)
    else:
        apply_gradient(param_groups, state, clip_grad, clip_grad_val, codec_.n_nodes)
    grads = [p.grad.data for p in params]
    bufs = None
    if mask_momentum and codec_.is_compress_op:
        bufs = [state[p].get("momentum_buffer") for p in params]
    values, indices, n_bits = codec_.compress(grads, memory_tb, compress_ratio, momentum_buffers=bufs,
                                              grads_in_memory=codec_.is_compress_op)
    synced, size = codec_.sync(values, indices)
    _, flatten_params = utils.recover_params(param_groups, param_names, get_hat_params=False)
    flatten_params.buffer = codec_.recover_info(flatten_params.buffer, synced, size, param_groups[0]["lr"])
    flatten_params.unpack([p.data for p in params])
    return n_bits
