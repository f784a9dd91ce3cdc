"""Drop-in for the ECD-PSGD compressor (dl_code/pcode/optim/ecd_psgd.py:186-455).

`ECDCompressor(aggregator=, comm_op=, comm_device=, compress_ratio=,
quantize_level=, is_biased=, backend=, use_ipc=)` with `.compress(sync_buffer)`
(input key `flatten_updated_params`: the extrapolated model, compressed as is),
`.sync(sync_buffer)` and `.uncompress(sync_buffer, neighbor_hat_params,
local_index)`, which extrapolates every neighbour replica with that neighbour's
message: hat <- (1 - 2/t) hat + (2/t) q  (t = local_index), in the reference's
rounding (mul, then torch's fused add with alpha; the sign receiver folds 2/t
into the per-tensor scale first, ecd_psgd.py:448-454).  Receivers are the
*_extrapolate kernels of include/choco_codec.h.

`fused_step(...)` is `ECD_PSGD.step` end to end (ecd_psgd.py:99-157): the batched
apply_gradient, one neighbour-mix launch for the updated params and the
extrapolated model (codec.params_mix), then compress / sync / uncompress;
`step_loop(...)` is the same step as one torch op per line (CPU tensors).
"""
import torch

from . import codec, utils
from .tensor_buffer import TensorBuffer
from .wire import _Facade, _QsgdConsumer, _SignConsumer, _SparseConsumer


def _finish(compressor, sync_buffer, neighbor_hat_params, local_index):
    compressor.compress(sync_buffer)
    compressor.sync(sync_buffer)
    compressor.uncompress(sync_buffer, neighbor_hat_params, local_index)
    return sync_buffer["n_bits"]


def step_loop(compressor, param_groups, param_names, state, shapes, neighbor_hat_params, neighbors_info, local_index):
    """ECD_PSGD.step (ecd_psgd.py:99-157) as the reference's op sequence, one torch op per line:
    the path CPU tensors, and anything the batched kernels do not take, keep."""
    entries = utils.step_entries(param_groups, param_names, "ecd.step_loop", need_grads=True)
    utils.apply_gradient_loop(param_groups, state, False)
    params = [p for _, p in entries]
    flatten_params = TensorBuffer([p.data for p in params], dtype=torch.float32)
    flatten_grads = TensorBuffer([p.grad.data for p in params], dtype=torch.float32)
    updated = TensorBuffer.from_flat(
        utils.weighted_sum([h.buffer for h in neighbor_hat_params.values()],
                           [neighbors_info[r] for r in neighbor_hat_params]), [p.size() for p in params])
    updated.buffer.add_(flatten_grads.buffer, alpha=-param_groups[0]["lr"])
    updated.unpack(params)
    updated.buffer = (1 - 0.5 * local_index) * flatten_params.buffer + 0.5 * local_index * updated.buffer
    sync_buffer = {"original_shapes": shapes, "flatten_updated_params": updated}
    return _finish(compressor, sync_buffer, neighbor_hat_params, local_index)


def fused_step(compressor, param_groups, param_names, state, shapes, neighbor_hat_params, neighbors_info, local_index,
               rounding=None):
    """ECD_PSGD.step end to end (ecd_psgd.py:99-157): the batched
    apply_gradient(apply_grad_to_model=False); ONE mix launch for :107-140, which writes the
    updated model sum(hat_r * w_r) + (-lr) * d_p (fused, as add_(alpha=)) into the params and
    the extrapolated model (1 - 0.5 t) * old params + 0.5 t * updated, t = local_index, into
    the buffer the compressor takes; this module's compress / sync / uncompress.  lr is
    param_groups[0]["lr"], as in the reference.  Returns n_bits.  Tensors the kernels do not
    take run step_loop."""
    utils.no_rounding("ecd.fused_step", rounding)  # stochastic rounding: not part of this step
    entries = utils.step_entries(param_groups, param_names, "ecd.fused_step", need_grads=True)
    plan = utils.grad_step_plan(entries, state, neighbor_hat_params)
    if plan is None:
        return step_loop(compressor, param_groups, param_names, state, shapes, neighbor_hat_params, neighbors_info,
                         local_index)
    updated = torch.empty(plan.n, dtype=torch.float32, device=plan.device)
    plan.mix([h.buffer for h in neighbor_hat_params.values()], [neighbors_info[r] for r in neighbor_hat_params],
             lr=param_groups[0]["lr"], mode=codec.MIX_GRAD_FMA | codec.MIX_WRITE_PARAMS | codec.MIX_EXTRAPOLATE,
             ext_a=1 - 0.5 * local_index, ext_b=0.5 * local_index, flat_out=updated)
    sync_buffer = {"original_shapes": shapes,
                   "flatten_updated_params": TensorBuffer.from_flat(updated, [p.size() for _, p in entries])}
    return _finish(compressor, sync_buffer, neighbor_hat_params, local_index)


def _coeffs(local_index):
    # Python doubles, rounded to fp32 where torch applies them to fp32 tensors
    return 1 - 2 / local_index, 2 / local_index


class _ECDInputs(object):
    """The extrapolated model, compressed as is (no x_hat)."""

    def _inputs(self, sync_buffer):
        x = sync_buffer["flatten_updated_params"].buffer
        return x, None, self._layout(sync_buffer, x.device)


class ECDSparsificationCompressor(_ECDInputs, _SparseConsumer):
    """top-k / random-k  (ecd_psgd.py:211-303)."""

    def compress(self, sync_buffer):
        self._sparse_message(sync_buffer, *self._inputs(sync_buffer))

    def uncompress(self, sync_buffer, neighbor_hat_params, local_index):
        a, b = _coeffs(local_index)
        for _, hat, (values, indices) in self._sparse_received(sync_buffer, self._replicas(neighbor_hat_params)):
            codec.sparse_extrapolate(values, indices, hat, a, b, guard=self._guards[hat.device])
        self._guards.sweep()


class ECDQuantizationCompressor(_ECDInputs, _QsgdConsumer):
    """QSGD  (ecd_psgd.py:306-423)."""

    def compress(self, sync_buffer):
        self._qsgd_message(sync_buffer, *self._inputs(sync_buffer))

    def uncompress(self, sync_buffer, neighbor_hat_params, local_index):
        q = int(self.quantize_level)
        a, b = _coeffs(local_index)
        for _, hat, msg in self._qsgd_received(sync_buffer, self._replicas(neighbor_hat_params)):
            if q == 32:
                hat.mul_(a).add_(msg, alpha=b)
                continue
            lay = self._layout(sync_buffer, hat.device)
            codec.qsgd_extrapolate(msg[0], msg[1], lay.n, q, hat, a, b, is_biased=self.is_biased,
                                   seg_off=lay.seg_off, nseg=lay.nseg)


class ECDSignCompressor(_ECDInputs, _SignConsumer):
    """sign + per-tensor L1 norm  (ecd_psgd.py:426-455)."""

    placeholder_key = "flatten_updates"

    def compress(self, sync_buffer):
        self._sign_message(sync_buffer, *self._inputs(sync_buffer))

    def uncompress(self, sync_buffer, neighbor_hat_params, local_index):
        a, b = _coeffs(local_index)
        for _, hat, (words, norms) in self._sign_received(sync_buffer, self._replicas(neighbor_hat_params)):
            lay = self._layout(sync_buffer, hat.device)
            codec.sign_extrapolate(words, norms, lay.n, hat, a, b, seg_off=lay.seg_off, nseg=lay.nseg)


class ECDCompressor(_Facade):
    sparsification, quantization, sign = ECDSparsificationCompressor, ECDQuantizationCompressor, ECDSignCompressor

