"""Drop-in for the DCD-PSGD compressor (dl_code/pcode/optim/dcd_psgd.py:150-446).

`DCDCompressor(aggregator=, comm_op=, comm_device=, compress_ratio=,
quantize_level=, is_biased=, backend=, use_ipc=)` with `.compress(sync_buffer)`,
`.sync(sync_buffer)`, `.uncompress(sync_buffer, neighbor_hat_params)`; input keys
`original_shapes`, `flatten_half_params`, `flatten_params`.  DCD compresses
d = half_params - params per tensor and every rank adds each neighbour's decoded
message into its replica of that neighbour's model (no memory, no weights).

Same primitives as the CHOCO drop-in (parallel_choco.py): one batched device
compress over the flat buffers and this codec's packed wire; the receiver is
the fused accumulate with weight 1 (x[idx] + 1.0f * v = x[idx] + v bit for bit;
the sign receiver uses torch's add_(u, alpha) rounding, dcd_psgd.py:446).  The
exchange keeps the reference's blocking `_agg(..., force_wait=True)` call.

`fused_step(...)` is `DCD_PSGD.step` end to end (dcd_psgd.py:96-144): the batched
apply_gradient, one neighbour-mix launch for the half params and the packed
params (codec.params_mix), then compress / sync / uncompress and the unpack;
`step_loop(...)` is the same step as one torch op per line (CPU tensors).
"""
import torch

from . import codec, utils
from .tensor_buffer import TensorBuffer
from .wire import _Facade, _QsgdConsumer, _SignConsumer, _SparseConsumer


def _own_rank(compressor):
    return getattr(compressor, "compressor_fn", compressor).aggregator_fn.rank


def _finish(compressor, sync_buffer, neighbor_hat_params, params):
    """compress, sync, uncompress, and the local model taken from this rank's own replica
    (dcd_psgd.py:127-144)."""
    compressor.compress(sync_buffer)
    compressor.sync(sync_buffer)
    compressor.uncompress(sync_buffer, neighbor_hat_params)
    return neighbor_hat_params[_own_rank(compressor)]


def step_loop(compressor, param_groups, param_names, state, shapes, neighbor_hat_params, neighbors_info):
    """DCD_PSGD.step (dcd_psgd.py:96-144) as the reference's op sequence, one torch op per line:
    the path CPU tensors, and anything the batched kernels do not take, keep."""
    entries = utils.step_entries(param_groups, param_names, "dcd.step_loop", need_grads=True)
    utils.apply_gradient_loop(param_groups, state, False)
    params = [p for _, p in entries]
    sizes = [p.size() for p in params]
    flatten_params = TensorBuffer([p.data for p in params], dtype=torch.float32)
    flatten_grads = TensorBuffer([p.grad.data for p in params], dtype=torch.float32)
    half = (utils.weighted_sum([h.buffer for h in neighbor_hat_params.values()],
                               [neighbors_info[r] for r in neighbor_hat_params])
            - param_groups[0]["lr"] * flatten_grads.buffer)
    sync_buffer = {"original_shapes": shapes, "flatten_half_params": TensorBuffer.from_flat(half, sizes),
                   "flatten_params": flatten_params}
    own = _finish(compressor, sync_buffer, neighbor_hat_params, params)
    flatten_params.buffer = own.buffer.clone()
    flatten_params.unpack(params)
    return sync_buffer["n_bits"]


def fused_step(compressor, param_groups, param_names, state, shapes, neighbor_hat_params, neighbors_info,
               rounding=None):
    """DCD_PSGD.step end to end (dcd_psgd.py:96-144): the batched
    apply_gradient(apply_grad_to_model=False); ONE mix launch for :104-125, which writes the
    half params sum(hat_r * w_r) - lr * d_p and packs the params beside them (the two inputs of
    the compressor); this module's compress / sync / uncompress; and the batched unpack
    straight from this rank's own replica (the reference clones it first).  lr is
    param_groups[0]["lr"], as in the reference.  Returns n_bits.  Tensors the kernels do not
    take run step_loop."""
    utils.no_rounding("dcd.fused_step", rounding)  # stochastic rounding: not part of this step
    entries = utils.step_entries(param_groups, param_names, "dcd.fused_step", need_grads=True)
    plan = utils.grad_step_plan(entries, state, neighbor_hat_params)
    if plan is None:
        return step_loop(compressor, param_groups, param_names, state, shapes, neighbor_hat_params, neighbors_info)
    params = [p for _, p in entries]
    sizes = [p.size() for p in params]
    half, packed = (torch.empty(plan.n, dtype=torch.float32, device=plan.device) for _ in range(2))
    plan.mix([h.buffer for h in neighbor_hat_params.values()], [neighbors_info[r] for r in neighbor_hat_params],
             lr=param_groups[0]["lr"], mode=codec.MIX_GRAD_SUB, flat_out=half, x_out=packed)
    sync_buffer = {"original_shapes": shapes, "flatten_half_params": TensorBuffer.from_flat(half, sizes),
                   "flatten_params": TensorBuffer.from_flat(packed, sizes)}
    _finish(compressor, sync_buffer, neighbor_hat_params, params).unpack(params)
    return sync_buffer["n_bits"]


class _DCDInputs(object):
    """d = half_params - params  (dcd_psgd.py:127-131)."""

    def _inputs(self, sync_buffer):
        x = sync_buffer["flatten_half_params"].buffer
        return x, sync_buffer["flatten_params"].buffer, self._layout(sync_buffer, x.device)


class DCDSparsificationCompressor(_DCDInputs, _SparseConsumer):
    """top-k / random-k  (dcd_psgd.py:175-275)."""

    def compress(self, sync_buffer):
        self._sparse_message(sync_buffer, *self._inputs(sync_buffer))

    def uncompress(self, sync_buffer, neighbor_hat_params):
        for _, hat, (values, indices) in self._sparse_received(sync_buffer, self._replicas(neighbor_hat_params)):
            # hat[idx] += v  (dcd_psgd.py:275) == hat[idx] + 1.0f * v
            codec.sparse_accumulate(values, indices, hat, 1.0, guard=self._guards[hat.device])
        self._guards.sweep()


class DCDQuantizationCompressor(_DCDInputs, _QsgdConsumer):
    """QSGD  (dcd_psgd.py:278-352)."""

    def compress(self, sync_buffer):
        self._qsgd_message(sync_buffer, *self._inputs(sync_buffer))

    def uncompress(self, sync_buffer, neighbor_hat_params):
        q = int(self.quantize_level)
        for _, hat, msg in self._qsgd_received(sync_buffer, self._replicas(neighbor_hat_params)):
            if q == 32:
                hat.add_(msg)
                continue
            lay = self._layout(sync_buffer, hat.device)
            # hat += decode(msg)  (dcd_psgd.py:352) == hat + 1.0f * v
            codec.qsgd_accumulate([msg], [1.0], -1, lay.n, q, hat, is_biased=self.is_biased, seg_off=lay.seg_off,
                                  nseg=lay.nseg)


class DCDSignCompressor(_DCDInputs, _SignConsumer):
    """sign + per-tensor L1 norm  (dcd_psgd.py:355-446)."""

    placeholder_key = "flatten_updates"

    def compress(self, sync_buffer):
        self._sign_message(sync_buffer, *self._inputs(sync_buffer))

    def uncompress(self, sync_buffer, neighbor_hat_params):
        for _, hat, msg in self._sign_received(sync_buffer, self._replicas(neighbor_hat_params)):
            lay = self._layout(sync_buffer, hat.device)
            # hat_s.add_(norm_s / numel_s, sign_s)  (dcd_psgd.py:442-446)
            codec.sign_axpy([msg], [1.0], lay.n, hat, seg_off=lay.seg_off, nseg=lay.nseg)


class DCDCompressor(_Facade):
    sparsification, quantization, sign = DCDSparsificationCompressor, DCDQuantizationCompressor, DCDSignCompressor
