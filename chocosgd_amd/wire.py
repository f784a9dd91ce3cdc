"""What the drop-in compressors share (parallel_choco.py, dcd.py, ecd.py, deep_squeeze.py,
ef_sign.py, dgc.py); each of those modules keeps what differs: where x / x_hat come from,
the key names, and the receiver call with its coefficients.

The wire FORMAT is codec.py's: `sparse_wire` / `sign_wire` / `qsgd_wire` build a message with
the views the kernels fill in place, `sparse_split` / `sign_split` / `qsgd_split` take a received
one apart.  Nothing here or in the drop-ins slices a message itself, but for the chunked
exchanges of parallel_choco.py, whose ranges are the unit that travels.

Here: the segment table of a parameter layout (`_Layout`), the `comm_op` facade, the nine-field
constructor, the host staging of a message, the three message builders with the `sync_buffer`
keys they write, the per-device guard cache, the consumers' three `sync` bodies and the receive
iteration.
"""
import torch

from . import codec
from .communication import recover_device
from .sparsification import _draw_seed, get_n_bits
from .tensor_buffer import TensorBuffer


def _seg_lens(original_shapes):
    return tuple(int(s[1]) for s in original_shapes)


class _Layout:
    """Device-side segment table + top-k plans for one parameter layout."""

    _cache = {}

    def __init__(self, lens, device):
        self.lens = lens
        self.nseg = len(lens)
        offs = [0]
        for s in lens:
            offs.append(offs[-1] + s)
        self.n = offs[-1]
        self.seg_off_list = offs
        self.seg_off = torch.tensor(offs, dtype=torch.int64, device=device) if self.nseg > 1 else None
        self.device = device
        self._plans = {}

    @classmethod
    def get(cls, lens, device):
        key = (lens, str(device))
        lay = cls._cache.get(key)
        if lay is None:
            lay = cls(lens, device)
            cls._cache[key] = lay
        return lay

    def topk_plan(self, ratio):
        p = self._plans.get(ratio)
        if p is None:
            p = codec.SegmentPlan(self.lens, ratio, self.device)
            self._plans[ratio] = p
        return p


_hdr_words = codec.wire_header_words  # int32 words of the fp32 norms header (16-byte aligned)


def _staged(message, comm_device):
    """The message as it is handed to the aggregator: in pinned host memory for comm_device
    "cpu" (parallel_choco_v.py:271-272)."""
    return message.cpu().pin_memory() if comm_device == "cpu" else message


def _received(synced, targets, split, *args):
    """One receive iteration: for every (rank or slot, target buffer) of `targets`, that
    entry of `synced` on the target's device, taken apart by codec's `split(message, *args)`."""
    for key, target in targets:
        yield key, target, split(recover_device(synced[key], device=target.device), *args)


class _Facade(object):
    """The public class of a family: picks the family's class for `comm_op` and forwards the
    three calls (explicit methods: they run every step)."""

    sparsification = quantization = sign = None  # the family's three classes

    def __init__(self, **kargs):
        if "top_k" in kargs["comm_op"] or "random_k" in kargs["comm_op"]:
            self.compressor_fn = self.sparsification(**kargs)
        elif "quantize" in kargs["comm_op"]:
            self.compressor_fn = self.quantization(**kargs)
        elif "sign" in kargs["comm_op"]:
            self.compressor_fn = self.sign(**kargs)
        else:
            raise NotImplementedError

    def compress(self, *args, **kargs):
        return self.compressor_fn.compress(*args, **kargs)

    def sync(self, *args, **kargs):
        return self.compressor_fn.sync(*args, **kargs)

    def uncompress(self, *args, **kargs):
        return self.compressor_fn.uncompress(*args, **kargs)


class _Guards(dict):
    """{device: codec.IndexGuard}, made on first use."""

    def __missing__(self, device):
        guard = self[device] = codec.IndexGuard(device)
        return guard

    def sweep(self):
        """End of a receive step: out-of-range indices of an EARLIER step (lazy, no sync) are
        reported once this step's messages are applied."""
        for guard in self.values():
            guard.check_then_arm()


class _LazyDict(dict):
    """A dict whose `self[r]` is computed on access: items / values go through it."""

    def items(self):
        return [(r, self[r]) for r in self.keys()]

    def values(self):
        return [self[r] for r in self.keys()]


class _SignSender(object):
    """The sign message [norms | words] and its keys.  The family names the TensorBuffer of
    the norms, the received norms, and the key of the delta it never materialises (fused)."""

    norms_key, synced_norms_key, placeholder_key = "flatten_norms", "synced_flatten_norms", None

    def _sign_message(self, sync_buffer, x, xh, lay, gossip=None, pending=None):
        """pending (CHOCO's deferred receive): called with (x, xh, gossip, lay) once the message
        exists; what it returns, if anything, is applied in the pass that packs."""
        message, (signs, norms) = codec.sign_wire(lay.n, lay.nseg, x.device)  # written in place by the kernels
        pend = pending(x, xh, gossip, lay) if pending is not None else None
        if pend is not None:  # the previous step's receive + the consensus step + the pack, one pass
            codec.sign_recv_gossip_compress(pend[0], pend[1], pend[2], x, gossip[0], xh, gossip[1],
                                            seg_off=lay.seg_off, nseg=lay.nseg, out=(signs, norms))
        else:
            codec.sign_compress(x, xhat=xh, seg_off=lay.seg_off, nseg=lay.nseg, want_norms=True, gossip=gossip,
                                out=(signs, norms))
        self._sign_keys(sync_buffer, message, signs, norms, lay)
        return signs, norms

    def _sign_keys(self, sync_buffer, message, signs, norms, lay):
        sync_buffer["sign_message"] = message
        sync_buffer[self.norms_key] = TensorBuffer.from_flat(norms, [() for _ in range(lay.nseg)])
        if self.placeholder_key is not None:
            sync_buffer[self.placeholder_key] = None
        sync_buffer["signs"] = signs
        sync_buffer["sign_size"] = torch.Size([lay.n])
        # nominal bits as in parallel_choco_v.py:492
        sync_buffer["n_bits"] = get_n_bits(norms) + get_n_bits(signs)

    def _sign_synced(self, sync_buffer, synced):
        """The reference's two received dicts (parallel_choco_v.py:521-522) as views of the one
        message per rank of `synced`."""
        nseg = sync_buffer[self.norms_key].buffer.numel()
        parts = {r: codec.sign_split(m, nseg) for r, m in synced.items()}
        sync_buffer["synced_message"] = synced
        sync_buffer[self.synced_norms_key] = {r: p[1] for r, p in parts.items()}
        sync_buffer["synced_signs"] = {r: p[0] for r, p in parts.items()}


class _Compressor(_SignSender):
    """The reference's nine constructor fields and the sparse and QSGD message builders."""

    def __init__(self, aggregator, comm_op, comm_device, compress_ratio, quantize_level, is_biased, backend,
                 use_ipc, **kargs):
        self.aggregator_fn = aggregator
        self.comm_op = comm_op
        self.comm_device = comm_device
        self.compress_ratio = compress_ratio
        self.quantize_level = quantize_level
        self.is_biased = is_biased
        self.backend = backend
        self.use_ipc = use_ipc
        self.kargs = kargs

    _draw_seed = staticmethod(_draw_seed)  # one draw from torch's generator per QSGD / random-k message

    @staticmethod
    def _layout(sync_buffer, device):
        return _Layout.get(_seg_lens(sync_buffer["original_shapes"]), device)

    # the codecs on a flat buffer x (d = x - xh when xh is given); gossip = (memory, gamma) fuses
    # the consensus step into the first pass
    def _sparse_message(self, sync_buffer, x, xh, lay, gossip=None):
        """values and GLOBAL int32 indices go straight into the message;
        `flatten_selected_indices` holds the reference's LOCAL per-tensor indices
        (parallel_choco_v.py:248-249), derived with the plan's cached segment starts."""
        plan = lay.topk_plan(float(self.compress_ratio))
        message, (values, indices) = codec.sparse_wire(plan.k_total, x.device)
        if "top_k" in self.comm_op:
            codec.topk_segmented(x, plan, xhat=xh, out=(values, indices), gossip=gossip)
        elif "random_k" in self.comm_op:
            # the reference never forwards is_biased to get_random_k (sparsification.py:60)
            codec.randk_segmented(x, plan, self._draw_seed(), is_biased=True, xhat=xh, out=(values, indices),
                                  gossip=gossip)
        else:
            raise NotImplementedError
        shapes = list(plan.k_per_seg)
        local = torch.sub(indices, plan.selected_base())
        sync_buffer["selected_shapes"] = shapes
        sync_buffer["flatten_selected_values"] = TensorBuffer.from_flat(values, [(k,) for k in shapes])
        sync_buffer["flatten_selected_indices"] = TensorBuffer.from_flat(local, [(k,) for k in shapes])
        sync_buffer["wire_message"] = message
        # nominal bits as in parallel_choco_v.py:252-254 (32-bit values + 32-bit indices)
        sync_buffer["n_bits"] = get_n_bits(values) + get_n_bits(local)
        return values, indices

    def _qsgd_message(self, sync_buffer, x, xh, lay, want_dense=False, gossip=None, pending=None):
        """Returns the dense decode (want_dense, or the delta itself at q == 32).  pending: as
        _sign_message's; its receive runs with the consensus step in the norm pass."""
        q = int(self.quantize_level)
        if q == 32:  # QuantizationCompressor passes the tensor through (sparsification.py:118-119)
            if gossip is not None:
                codec.gossip_step(x, gossip[0], xh, gossip[1])
            dense = torch.sub(x, xh) if xh is not None else x
            message = dense.contiguous().view(torch.uint8)
        else:
            message, out = codec.qsgd_wire(lay.n, q, lay.nseg, x.device)  # written in place by the kernels
            norm_in = None
            pend = pending(x, xh, gossip, lay) if pending is not None else None
            if pend is not None:
                # the previous step's receive + the consensus step + the norm pass, one kernel;
                # then the quantize pass with those norms
                codec.qsgd_recv_gossip_norms(pend[0], pend[1], pend[2], x, gossip[0], xh, gossip[1], q,
                                             is_biased=self.is_biased, seg_off=lay.seg_off, nseg=lay.nseg,
                                             out=out[1])
                gossip, norm_in = None, out[1]
            _, _, dense = codec.qsgd_compress(x, q, is_biased=self.is_biased, xhat=xh, seg_off=lay.seg_off,
                                              nseg=lay.nseg, norm_in=norm_in, seed=self._draw_seed(),
                                              want_dense=want_dense, gossip=gossip, out=out)
        self._qsgd_keys(sync_buffer, x, message)
        return dense

    def _qsgd_keys(self, sync_buffer, x, message):
        sync_buffer["flatten_updates"] = TensorBuffer.from_flat(message, [(message.numel(),)])
        # nominal bits as in parallel_choco_v.py:393
        sync_buffer["n_bits"] = get_n_bits(x) * self.quantize_level / 32
        sync_buffer["n_bits_wire"] = 8 * message.numel()

    # one receive iteration per codec: (rank, target, split message) for every (rank, target
    # buffer) of `targets`, from the `synced_message` of the family's sync
    def _sparse_received(self, sync_buffer, targets):
        """(values, indices) per target; the caller sweeps its guards after the loop."""
        return _received(sync_buffer["synced_message"], targets, codec.sparse_split,
                         sync_buffer["sycned_message_size"])

    def _qsgd_received(self, sync_buffer, targets):
        """(planes, norms) per target, or the raw delta at q == 32."""
        if int(self.quantize_level) == 32:
            return _received(sync_buffer["synced_message"], targets, lambda m: m.view(torch.float32))
        return _received(sync_buffer["synced_message"], targets, codec.qsgd_split,
                         len(sync_buffer["original_shapes"]))

    def _sign_received(self, sync_buffer, targets):
        """(words, norms) per target."""
        return _received(sync_buffer["synced_message"], targets, codec.sign_split,
                         len(sync_buffer["original_shapes"]))


class _Consumer(_Compressor):
    """The non-CHOCO consumers (DCD, ECD, DeepSqueeze): the reference's blocking exchange, and
    `sync` per codec in the three classes below.  A family's class derives from one of them."""

    def _send(self, message):
        return self.aggregator_fn._agg(_staged(message, self.comm_device), op="get_raw_sync_data", force_wait=True)

    @staticmethod
    def _replicas(neighbor_hat_params):
        """The receive targets of DCD and ECD: every neighbour's replica, each on its own device."""
        return ((rank, hat.buffer) for rank, hat in neighbor_hat_params.items())


class _SparseConsumer(_Consumer):
    def __init__(self, *args, **kargs):
        super().__init__(*args, **kargs)
        self._guards = _Guards()

    def sync(self, sync_buffer):
        message = sync_buffer["wire_message"]
        sync_buffer["synced_message"] = self._send(message)
        sync_buffer["sycned_message_size"] = len(message)


class _QsgdConsumer(_Consumer):
    def sync(self, sync_buffer):
        sync_buffer["synced_message"] = self._send(sync_buffer["flatten_updates"].buffer)


class _SignConsumer(_Consumer):
    """Norms and signs travel in ONE message; the received norms / `synced_signs` are views of it."""

    def sync(self, sync_buffer):
        self._sign_synced(sync_buffer, self._send(sync_buffer["sign_message"]))
