"""Drop-in for the DeepSqueeze compressor (dl_code/pcode/optim/deep_squeeze.py:133-489).

`DeepSqueezeCompressor(aggregator=, rank=, comm_op=, comm_device=, compress_ratio=,
quantize_level=, is_biased=, backend=, use_ipc=, consensus_stepsize=)`:
  * `.compress(sync_buffer)` compresses the error-compensated memory
    `sync_buffer["params_tb"]` and RETURNS the local compressed copy (the
    decoded message as this rank sees it) as a TensorBuffer -- the caller's
    error feedback is `memory - local` (deep_squeeze.py:110-115);
  * `.sync(sync_buffer)` exchanges with the reference's blocking `_agg`;
  * `.uncompress(sync_buffer, neighbors_info)` RETURNS
    sum_r consensus_stepsize * (w_r - [r == rank]) * decode(msg_r).

Device side: the same batched codec as CHOCO / DCD; the local copy comes from
kernels (top-k: a scatter of the message into zeros with the accumulate kernel,
QSGD: the quantize pass's dense decode, sign: choco_sign_local_decode with
torch.sign's sign(0) = 0); the aggregate uses the receivers with the
reference's two-rounding add_(c * u) (include/choco_codec.h).

`fused_step(...)` is `DeepSqueeze.step` end to end (deep_squeeze.py:94-127): the batched
apply_gradient, `memory += params` straight from the parameter tensors
(codec.params_ef), `compress(sync_buffer, residual=True)` -- the message, then
`memory -= local copy` in place with no local copy built --, sync / uncompress, and
`params += aggregate` straight into the parameter tensors.  `step_loop(...)` is the same
step as one torch op per line (CPU tensors).
"""
import torch

from . import codec, utils
from .tensor_buffer import TensorBuffer
from .wire import _Consumer, _Facade, _QsgdConsumer, _SignConsumer, _SparseConsumer


def step_loop(compressor, param_groups, param_names, state, shapes, memory, neighbors_info):
    """DeepSqueeze.step (deep_squeeze.py:94-127) as the reference's op sequence, one torch op per
    line: the path CPU tensors, and anything the batched kernels do not take, keep."""
    entries = utils.step_entries(param_groups, param_names, "deep_squeeze.step_loop")
    utils.apply_gradient(param_groups, state, apply_grad_to_model=True)
    params = [p for _, p in entries]
    params_tb = TensorBuffer([p.data for p in params], dtype=torch.float32)
    memory.buffer += params_tb.buffer
    sync_buffer = {"original_shapes": shapes, "params_tb": memory}
    local_compressed_params_tb = compressor.compress(sync_buffer)
    memory.buffer = memory.buffer - local_compressed_params_tb.buffer
    compressor.sync(sync_buffer)
    aggregated_info_tb = compressor.uncompress(sync_buffer, neighbors_info)
    params_tb.buffer += aggregated_info_tb.buffer
    params_tb.unpack(params)
    return sync_buffer["n_bits"]


def fused_step(compressor, param_groups, param_names, state, shapes, memory, neighbors_info, rounding=None):
    """DeepSqueeze.step end to end (deep_squeeze.py:94-127): the batched
    apply_gradient(apply_grad_to_model=True) writes the params; ONE params_ef launch (per chunk)
    adds them onto memory.buffer (:101-108, no flat copy of the params); the compressor builds
    its message and subtracts its local copy from memory.buffer in place
    (compress(residual=True), :110-115); sync and uncompress as they are; ONE params_ef launch
    adds the aggregate onto the params (:125-126).  No pack, no unpack.  memory.buffer is
    updated in place, where the reference rebinds it.  Returns n_bits.  Tensors the kernels do
    not take run step_loop."""
    utils.no_rounding("deep_squeeze.fused_step", rounding)  # stochastic rounding: not part of this step
    entries = utils.step_entries(param_groups, param_names, "deep_squeeze.fused_step")
    mem = memory.buffer
    plan = utils._sgd_fill(entries, state, True, mem) if mem.is_cuda else None
    if plan is None:
        return step_loop(compressor, param_groups, param_names, state, shapes, memory, neighbors_info)
    plan.run(None, grad_mode=False, write=True)
    plan.ef(mem, codec.EF_ACCUM)
    sync_buffer = {"original_shapes": shapes, "params_tb": memory}
    compressor.compress(sync_buffer, residual=True)
    compressor.sync(sync_buffer)
    agg = compressor.uncompress(sync_buffer, neighbors_info)
    plan.ef(agg.buffer, codec.EF_APPLY)
    return sync_buffer["n_bits"]




class _DeepSqueezeBase(_Consumer):
    norms_key, synced_norms_key = "param_norms_tb", "synced_param_norms"

    def __init__(self, aggregator, rank, comm_op, comm_device, compress_ratio, quantize_level, is_biased, backend,
                 use_ipc, consensus_stepsize, **kargs):
        super().__init__(aggregator, comm_op, comm_device, compress_ratio, quantize_level, is_biased, backend,
                         use_ipc, **kargs)
        self.rank = rank
        self.consensus_stepsize = consensus_stepsize

    def _inputs(self, sync_buffer):
        """The error-compensated memory, compressed as is (no x_hat)."""
        tb = sync_buffer["params_tb"]
        x = tb.buffer
        lay = self._layout(sync_buffer, x.device)
        if lay.n != x.numel():
            raise RuntimeError("original_shapes do not match params_tb")
        return tb, x, lay

    def _aggregate(self, sync_buffer, neighbors_info, received):
        """params_tb, zeros like it, and the codec's receive iteration over the neighbours into them."""
        tb = sync_buffer["params_tb"]
        agg = torch.zeros_like(tb.buffer)
        return tb, agg, received(sync_buffer, ((rank, agg) for rank in neighbors_info.keys()))

    def _weight(self, neighbors_info, rank):
        # deep_squeeze.py:275-277 -- a Python double, rounded to fp32 where torch multiplies
        return self.consensus_stepsize * (neighbors_info[rank] - (1 if rank == self.rank else 0))

    @staticmethod
    def _like(tb, buffer):
        return TensorBuffer.from_flat(buffer, tb._tensors_sizes)


class DeepSqueezeSparsificationCompressor(_DeepSqueezeBase, _SparseConsumer):
    """top-k / random-k  (deep_squeeze.py:158-279)."""

    def compress(self, sync_buffer, residual=False):
        """residual: params_tb.buffer -= local copy in place, at the selected positions only
        (m + (-v) is m - v bit for bit, m - 0 = m everywhere else); returns None."""
        tb, x, lay = self._inputs(sync_buffer)
        values, indices = self._sparse_message(sync_buffer, x, None, lay)
        if residual:
            codec.sparse_accumulate(values, indices, x, -1.0)
            return None
        local = torch.zeros_like(x)
        codec.sparse_accumulate(values, indices, local, 1.0)  # local[idx] = v  (deep_squeeze.py:206-208)
        return self._like(tb, local)

    def uncompress(self, sync_buffer, neighbors_info):
        tb, agg, received = self._aggregate(sync_buffer, neighbors_info, self._sparse_received)
        for rank, _, (values, indices) in received:
            # agg[idx] += c * v  (two roundings, deep_squeeze.py:274-278)
            codec.sparse_accumulate(values, indices, agg, self._weight(neighbors_info, rank),
                                    guard=self._guards[agg.device])
        self._guards.sweep()
        return self._like(tb, agg)


class DeepSqueezeQuantizationCompressor(_DeepSqueezeBase, _QsgdConsumer):
    """QSGD  (deep_squeeze.py:282-376)."""

    def compress(self, sync_buffer, residual=False):
        """residual: params_tb.buffer -= the dense decode in place; returns None."""
        tb, x, lay = self._inputs(sync_buffer)
        dense = self._qsgd_message(sync_buffer, x, None, lay, want_dense=True)
        if residual:
            if int(self.quantize_level) == 32:  # the message is a view of x: it keeps its own bytes
                wire = sync_buffer["flatten_updates"]
                wire.buffer = wire.buffer.clone()
            x.sub_(dense)
            return None
        return self._like(tb, dense.clone() if int(self.quantize_level) == 32 else dense)

    def uncompress(self, sync_buffer, neighbors_info):
        tb, agg, received = self._aggregate(sync_buffer, neighbors_info, self._qsgd_received)
        lay = self._layout(sync_buffer, agg.device)
        q = int(self.quantize_level)
        for rank, _, msg in received:
            c = self._weight(neighbors_info, rank)
            if q == 32:
                agg.add_(c * msg)
                continue
            # agg += c * decode(msg)  (two roundings, deep_squeeze.py:371-375)
            codec.qsgd_accumulate([msg], [c], -1, lay.n, q, agg, is_biased=self.is_biased, seg_off=lay.seg_off,
                                  nseg=lay.nseg)
        return self._like(tb, agg)


class DeepSqueezeSignCompressor(_DeepSqueezeBase, _SignConsumer):
    """sign + per-tensor L1 norm  (deep_squeeze.py:379-489)."""

    def compress(self, sync_buffer, residual=False):
        """residual: params_tb.buffer -= local copy in place, in the pass that decodes it
        (codec.sign_local_residual); returns None."""
        tb, x, lay = self._inputs(sync_buffer)
        _, norms = self._sign_message(sync_buffer, x, None, lay)
        if residual:
            codec.sign_local_residual(x, norms, seg_off=lay.seg_off, nseg=lay.nseg, resid_out=x)
            return None
        # (norm_s * torch.sign(x)) / numel_s  (deep_squeeze.py:416-422)
        local = codec.sign_local_decode(x, norms, seg_off=lay.seg_off, nseg=lay.nseg)
        return self._like(tb, local)

    def uncompress(self, sync_buffer, neighbors_info):
        tb, agg, received = self._aggregate(sync_buffer, neighbors_info, self._sign_received)
        lay = self._layout(sync_buffer, agg.device)
        for rank, _, msg in received:
            # agg_s.add_(c * (norm_s / numel_s * sign_s))  (two roundings, deep_squeeze.py:481-488)
            codec.sign_axpy([msg], [self._weight(neighbors_info, rank)], lay.n, agg, seg_off=lay.seg_off,
                            nseg=lay.nseg, two_roundings=True)
        return self._like(tb, agg)


class DeepSqueezeCompressor(_Facade):
    sparsification, quantization, sign = (DeepSqueezeSparsificationCompressor, DeepSqueezeQuantizationCompressor,
                                          DeepSqueezeSignCompressor)
