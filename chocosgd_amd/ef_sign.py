"""Drop-in for the EF-signSGD compressor (dl_code/pcode/optim/ef_sign_sgd.py:126-219).

`EFSignCompressor(rank, world_size, aggregator, comm_op, comm_device, use_ipc)`:
  * `.compress(grads_tb)` -> sync_buffer with the per-tensor L1 norms, the packed
    signs and `synced_grads_tb` = this rank's decoded copy (norm * sign(g) / numel,
    sign(0) = 0) that the optimizer's error feedback subtracts;
  * `.sync(sync_buffer)` all-gathers ONE [norms | words] message per rank through a
    centralized aggregator (`_agg(..., communication_scheme="all_gather")`);
  * `.decompress(sync_buffer)` adds every other rank's decoded signs (in rank
    order) and divides by the world size.
Kernels: the batched sign pack (norms fused), choco_sign_local_decode and the
fused multi-message sign receiver (weight 1).

`fused_step(...)` is `EF_SignSGD.step` end to end (ef_sign_sgd.py:78-123): the batched
apply_gradient that adds d_p onto the memory in the same pass, the sign pack, the local copy
and `memory = grads - local` in one pass (codec.sign_local_residual), sync, the receiver, and
ONE codec.params_ef launch for `/= world_size`, `-lr *` and the add into the parameter
tensors.  `step_loop(...)` is the same step as one torch op per line (CPU tensors).
"""
import torch

from . import codec, utils
from .tensor_buffer import TensorBuffer
from .wire import _Layout, _SignSender, _received, _staged


def step_loop(compressor, param_groups, param_names, state, memory_tb):
    """EF_SignSGD.step (ef_sign_sgd.py:78-123) as the reference's op sequence, one torch op per
    line: the path CPU tensors, and anything the batched kernels do not take, keep."""
    entries = utils.step_entries(param_groups, param_names, "ef_sign.step_loop", need_grads=True)
    utils.apply_gradient(param_groups, state, apply_grad_to_model=False)
    params = [p for _, p in entries]
    grads_tb = TensorBuffer([p.grad.data for p in params], dtype=torch.float32)
    grads_tb.buffer.add_(memory_tb.buffer)
    sync_buffer = compressor.compress(grads_tb)
    compressor.sync(sync_buffer)
    memory_tb.buffer = grads_tb.buffer - sync_buffer["synced_grads_tb"].buffer
    sync_grads_tb = compressor.decompress(sync_buffer)
    params_tb = TensorBuffer([p.data for p in params], dtype=torch.float32)
    params_tb.buffer.add_(-param_groups[0]["lr"] * sync_grads_tb.buffer)
    params_tb.unpack(params)
    return sync_buffer["n_bits"]


def fused_step(compressor, param_groups, param_names, state, memory_tb, rounding=None):
    """EF_SignSGD.step end to end (ef_sign_sgd.py:78-123): the batched
    apply_gradient(apply_grad_to_model=False) writes d_p into the grads and adds it onto
    memory_tb.buffer in the same pass (:79-93; the buffer now holds d_p + memory, no flat copy
    of the grads); the sign pack with norms; ONE pass writes this rank's decoded copy into
    synced_grads and leaves grads - copy, the new memory, in memory_tb.buffer (:153, :104-106;
    compress(residual=True)); sync; the receiver without its division
    (decompress(divide=False)); ONE params_ef launch (per chunk) divides synced_grads by the
    world size, scales by -lr and adds into the params (:218, :113-122).  No pack, no unpack.
    memory_tb.buffer is updated in place, where the reference rebinds it.  lr is
    param_groups[0]["lr"], as in the reference.  Returns n_bits.  Tensors the kernels do not take
    run step_loop."""
    utils.no_rounding("ef_sign.fused_step", rounding)  # stochastic rounding: not part of this step
    entries = utils.step_entries(param_groups, param_names, "ef_sign.fused_step", need_grads=True)
    mem = memory_tb.buffer
    plan = utils._sgd_fill(entries, state, False, mem) if mem.is_cuda else None
    if plan is None:
        return step_loop(compressor, param_groups, param_names, state, memory_tb)
    plan.run(mem, grad_mode=True, write=True, add_flat=True)
    sync_buffer = compressor.compress(memory_tb, residual=True)
    compressor.sync(sync_buffer)
    synced = compressor.decompress(sync_buffer, divide=False)
    plan.ef(synced.buffer, codec.EF_APPLY | codec.EF_DIV | codec.EF_SCALE, lr=param_groups[0]["lr"],
            divisor=compressor.world_size * 1.0)
    return sync_buffer["n_bits"]


class EFSignCompressor(_SignSender):
    norms_key = "grad_norms_tb"

    def __init__(self, rank, world_size, aggregator, comm_op, comm_device, use_ipc, **kargs):
        self.rank = rank
        self.world_size = world_size
        self.aggregator_fn = aggregator
        self.comm_op = comm_op
        self.comm_device = comm_device
        self.use_ipc = use_ipc
        self.kargs = kargs

    @staticmethod
    def _layout(tb):
        lens = tuple(int(torch.Size(s).numel()) for s in tb._tensors_sizes)
        return _Layout.get(lens, tb.buffer.device)

    def compress(self, grads_tb, residual=False):
        """residual: grads_tb.buffer is left holding grads - local copy (the new memory of
        ef_sign_sgd.py:104-106), written in the pass that decodes the copy."""
        g = grads_tb.buffer
        lay = self._layout(grads_tb)
        sync_buffer = {"grads_tb": grads_tb}
        _, norms = self._sign_message(sync_buffer, g, None, lay)
        if residual:
            local = torch.empty_like(g)
            codec.sign_local_residual(g, norms, seg_off=lay.seg_off, nseg=lay.nseg, local_out=local, resid_out=g)
        else:
            local = codec.sign_local_decode(g, norms, seg_off=lay.seg_off, nseg=lay.nseg)
        sync_buffer["synced_grads_tb"] = TensorBuffer.from_flat(local, grads_tb._tensors_sizes)
        return sync_buffer

    def sync(self, sync_buffer):
        # [norms | signs]: written in place by compress
        synced = self.aggregator_fn._agg(_staged(sync_buffer["sign_message"], self.comm_device),
                                         communication_scheme="all_gather", async_op=False)
        # the all-gather's list in rank order, where the neighbour exchanges give a dict
        parts = [codec.sign_split(m, len(sync_buffer["grad_norms_tb"])) for m in synced]
        sync_buffer["synced_message"] = synced
        sync_buffer["synced_grad_norms"] = [norms for _, norms in parts]
        sync_buffer["synced_signs"] = [words for words, _ in parts]

    def decompress(self, sync_buffer, divide=True):
        """divide=False: the sum is left undivided (the caller's params_ef(EF_DIV) divides it)."""
        tb = sync_buffer["synced_grads_tb"]
        dev = tb.buffer.device
        lay = self._layout(tb)
        others = ((rank, tb.buffer) for rank in range(self.world_size) if rank != self.rank)
        parts = [msg for _, _, msg in _received(sync_buffer["synced_message"], others, codec.sign_split, lay.nseg)]
        if parts:
            # synced_grad_s.add_(norm_s * sign_s / numel_s)  (ef_sign_sgd.py:212-215), ranks in order
            codec.sign_axpy(parts, [1.0] * len(parts), lay.n, tb.buffer, seg_off=lay.seg_off, nseg=lay.nseg)
        if not divide:
            return tb
        # true division (a device 0-dim divisor: torch multiplies by the reciprocal of a CPU scalar)
        tb.buffer.div_(torch.full((), self.world_size * 1.0, dtype=torch.float32, device=dev))
        return tb
