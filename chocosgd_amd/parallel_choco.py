"""Drop-in for the CHOCO compressor operator API of
dl_code/pcode/optim/parallel_choco_v.py:158-558 (byte-identical copy in
parallel_choco.py:209-609).

`CHOCOCompressor(aggregator=, comm_op=, comm_device=, compress_ratio=,
quantize_level=, is_biased=, backend=, use_ipc=)` with `.pipeline / .compress /
.sync / .uncompress(sync_buffer, neighbor_hat_params, neighbors_info)` and the
same `sync_buffer` contract: input keys `original_shapes`, `flatten_params`,
`flatten_hat_params`; `n_bits` is the reference's nominal bit count.

What changes underneath:
  * compress is ONE fused device pass over the whole flat buffer (delta
    x - x_hat, per-tensor selection / quantization / sign + L1 norms) instead of
    a Python loop over parameter tensors plus TensorBuffer copies;
  * the wire is this codec's packed format: top-k = [fp32 values | int32 GLOBAL
    indices] (exact beyond 2^24, unlike the reference's fp32 indices);
    QSGD = [fp32 norms | level plane | sign plane]; sign = [fp32 norms | packed
    words] in ONE message (the reference sends norms and signs separately);
  * uncompress applies all neighbour messages with fused kernels in
    `neighbors_info` order, reproducing the reference's fp32 rounding sequence;
  * optional input key `gossip` = (memory buffer, consensus_stepsize): compress
    first applies ParallelCHOCO_V.step's update_params_from_neighbor
    (optim/utils.py:67-72) to `flatten_params` inside its own first pass
    (utils.fused_step drives it; include/choco_codec.h "fused gossip step");
  * optional input key `defer_receive` (QSGD, sign): uncompress keeps the received
    messages and the NEXT compress applies them in the same pass as its consensus step
    (include/choco_codec.h "deferred receive"); x_hat / memory lag by one step until that
    compress or `flush_receive()` (utils.fused_step(defer_receive=True) drives it).
"""
import contextlib
import inspect

import torch

from . import codec
from .communication import recover_device
from .sparsification import _draw_seed
from .wire import _Compressor, _Facade, _Guards, _LazyDict, _hdr_words, _received, _staged


class _CHOCOBase(_Compressor):
    def __init__(self, *args, **kargs):
        super().__init__(*args, **kargs)
        # the reference binds the current stream here (parallel_choco_v.py:214-218)
        self.gossip_stream = torch.cuda.current_stream()
        # deferred receive: (messages, weights, self slot, memory, x_hat_i, layout) that the
        # next compress applies in its first pass (or flush_receive() applies alone)
        self._pending = None

    def _draw_seed(self):
        return _draw_seed()  # this module's name, looked up per call: callers pin per-worker seeds through it

    @contextlib.contextmanager
    def _on_gossip_stream(self):
        """Run the body on the gossip stream, ordered after everything the caller's current
        stream holds so far, and make the caller's stream wait for it on the way out (an error
        included).  The reference binds the gossip stream at construction; a caller that steps
        under another stream hands x / x_hat / memory over in both directions.  With the
        caller already on the gossip stream nothing is queued at all."""
        caller = torch.cuda.current_stream(self.gossip_stream.device)
        if caller == self.gossip_stream:
            yield
            return
        self.gossip_stream.wait_stream(caller)
        try:
            with torch.cuda.stream(self.gossip_stream):
                yield
        finally:
            caller.wait_stream(self.gossip_stream)

    def pipeline(self, sync_buffer, neighbor_hat_params, neighbors_info):
        # misuse, not a transport error: raised to the caller with nothing launched and the
        # pending receive kept (inside the try it would be printed, and every later step would
        # print it again and train without gossip)
        self._require_fused_consensus(self._gossip(sync_buffer))
        with self._on_gossip_stream():
            try:
                self.compress(sync_buffer)
                self.sync(sync_buffer)
                self.uncompress(sync_buffer, neighbor_hat_params, neighbors_info)
            except RuntimeError as e:
                print("Error: {}".format(e))

    # helpers --------------------------------------------------------------
    def _flat_inputs(self, sync_buffer):
        x = sync_buffer["flatten_params"].buffer
        xh = sync_buffer["flatten_hat_params"].buffer
        lay = self._layout(sync_buffer, x.device)
        if lay.n != x.numel():
            raise RuntimeError("original_shapes do not match flatten_params")
        return x, xh, lay

    @staticmethod
    def _gossip(sync_buffer):
        g = sync_buffer.get("gossip")
        return None if g is None else (g[0], float(g[1]))

    def _send(self, sync_buffer, message, out=None):
        message = _staged(message, self.comm_device)
        if out is None:
            return self.aggregator_fn._agg(message, op="get_raw_sync_data", force_wait=False)
        return self.aggregator_fn._agg(message, op="get_raw_sync_data", force_wait=False, out=out)

    def _receive_plan(self, sync_buffer, neighbor_hat_params, neighbors_info):
        """The neighbour ranks in `neighbors_info` order and, as _apply / _defer take them after
        the messages: their weights, the slot of this rank's own message (-1: none), memory,
        x_hat_i and the layout."""
        memory = neighbor_hat_params["memory"].buffer
        lay = self._layout(sync_buffer, memory.device)
        ranks = list(neighbors_info.keys())
        weights = [neighbors_info[r] for r in ranks]
        self_slot = self._self_slot(ranks, neighbor_hat_params)
        xhat_self = neighbor_hat_params[ranks[self_slot]].buffer if self_slot >= 0 else None
        return ranks, (weights, self_slot, memory, xhat_self, lay)

    # deferred receive ---------------------------------------------------------
    def _defer(self, parts, weights, self_slot, memory, xhat_self, lay):
        if self._pending is not None:
            raise RuntimeError("deferred receive: the previous step's messages were never applied")
        self._pending = (parts, weights, self_slot, memory, xhat_self, lay)

    def _require_fused_consensus(self, g):
        """A pending receive may only be applied by a compress whose first pass runs the
        consensus step itself (then that pass reads x_hat / memory after the receive).  With
        the consensus step run outside (g is None: the reference's ParallelCHOCO_V.step),
        recover_params and update_params_from_neighbor have already read the stale x_hat and
        memory, so x and this step's message would silently diverge from the reference."""
        if self._pending is not None and g is None:
            raise RuntimeError("deferred receive pending: call compressor.flush_receive() before recover_params / "
                               "update_params_from_neighbor (the previous step ran with defer_receive=True)")

    def _flush_before_pass(self, g):
        """Compress paths that never take a receive into their own pass: apply a pending one
        first (valid only with the consensus step fused into this compress)."""
        self._require_fused_consensus(g)
        self.flush_receive()

    def _take_pending(self, x, xh, g, lay):
        """The message builders' `pending` hook: the pending receive if this compress can apply
        it in its first pass (the consensus step fused, x_hat_i itself -- not a copy -- as
        flatten_hat_params); otherwise it is applied on its own first (flush_receive; the fused
        consensus step then reads the updated x_hat / memory), and None.  Raises when the
        consensus step is not fused into this compress (_require_fused_consensus)."""
        pend = self._pending
        if pend is None:
            return None
        self._require_fused_consensus(g)
        parts, weights, slot, memory, xhat_self, play = pend
        if play is not lay:
            self.flush_receive()
            return None
        if g[0].data_ptr() != memory.data_ptr() or (slot >= 0 and xh.data_ptr() != xhat_self.data_ptr()):
            raise RuntimeError("deferred receive: the next compress must take the same memory buffer and x_hat_i "
                               "itself as flatten_hat_params (utils.fused_step(defer_receive=True))")
        self._pending = None
        return parts, weights, slot

    def flush_receive(self):
        """Apply a deferred receive now (before reading x_hat / memory between steps).  It runs
        on the gossip stream, where the pending messages, memory and x_hat were written; the
        caller's current stream waits for it, so x_hat / memory may be read there right after."""
        pend, self._pending = self._pending, None
        if pend is not None:
            with self._on_gossip_stream():
                self._apply(*pend)

    @staticmethod
    def _self_slot(ranks, neighbor_hat_params):
        slots = [i for i, r in enumerate(ranks) if r in neighbor_hat_params]
        if len(slots) > 1:
            raise RuntimeError("more than one local x_hat in neighbor_hat_params")
        return slots[0] if slots else -1


class CHOCOSparsificationCompressor(_CHOCOBase):
    """top-k / random-k  (parallel_choco_v.py:189-332); the message and its keys are
    wire._sparse_message's."""

    def __init__(self, *args, **kargs):
        super().__init__(*args, **kargs)
        self._guards = _Guards()

    def compress(self, sync_buffer):
        x, xh, lay = self._flat_inputs(sync_buffer)
        self._sparse_message(sync_buffer, x, xh, lay, gossip=self._gossip(sync_buffer))

    def sync(self, sync_buffer):
        message = sync_buffer["wire_message"]
        reqs, synced = self._send(sync_buffer, message)
        sync_buffer["sync_reqs"] = reqs
        sync_buffer["synced_message"] = synced
        sync_buffer["sycned_message_size"] = len(message)

    def uncompress(self, sync_buffer, neighbor_hat_params, neighbors_info):
        # Not the consumers' receive loop: x_hat's scatter is queued before the wait in the
        # middle, and one call then takes every message (no _receive_plan either: x_hat's slot
        # depends on that early scatter).
        memory = neighbor_hat_params["memory"].buffer
        guard = self._guards[memory.device]
        # x_hat takes only the local message (hat_params.buffer += q_values,
        # parallel_choco_v.py:307-308): with remote messages pending, its scatter is
        # queued BEFORE waiting for them, so it runs while the exchange is in flight.
        # Bit-identical: memory's updates keep the neighbour order below.
        local = [r for r in neighbors_info if r in neighbor_hat_params]
        hat_early = len(local) == 1 and len(neighbors_info) > 1
        if hat_early:
            values, indices = codec.sparse_split(sync_buffer["wire_message"], sync_buffer["sycned_message_size"])
            codec.sparse_accumulate(values, indices, neighbor_hat_params[local[0]].buffer, 1.0, guard=guard)
        self.aggregator_fn.complete_wait(sync_buffer["sync_reqs"])
        # every message applied by ONE call that runs the per-message kernels in neighbors_info
        # order (bit-identical to the reference's per-neighbour loop); a merged one-sweep form
        # was measured slower and removed ("Sparse accumulate")
        targets = ((r, neighbor_hat_params[r if r in neighbor_hat_params else "memory"].buffer) for r in neighbors_info)
        msgs, slot, hat = [], -1, None
        for rank, target, msg in self._sparse_received(sync_buffer, targets):
            if rank in neighbor_hat_params and not hat_early:
                slot, hat = len(msgs), target
            msgs.append(msg)
        codec.sparse_accumulate_multi(msgs, list(neighbors_info.values()), memory, self_slot=slot, xhat_self=hat,
                                      guard=guard)
        # pipeline() prints what the sweep reports as the reference prints its RuntimeErrors
        self._guards.sweep()

    def check(self, wait=True):
        """Report bad received indices now (teardown / checkpoint): raises RuntimeError."""
        for g in self._guards.values():
            g.check(wait=wait)


class CHOCOQuantizationCompressor(_CHOCOBase):
    """QSGD  (parallel_choco_v.py:335-433).

    `exchange_chunks=C` (> 1, a constructor keyword every rank must pass alike) pipelines
    the exchange (communication.py:259-262): the norm pass, then C element
    ranges each quantized and SENT as soon as it is packed (the transfer of range c overlaps
    the quantize of range c + 1), and uncompress decodes range c as soon as it has arrived
    (overlapping the transfer of c + 1).  The wire is the chunked form of
    codec.qsgd_chunked_wire; x_hat / memory are bit-identical to C = 1 (every element sees
    the same messages in the same neighbour order).  `synced_message[rank]` is then the list
    [norms header, range 0, range 1, ...]."""

    def __init__(self, *args, **kargs):
        super().__init__(*args, **kargs)
        self.exchange_chunks = int(self.kargs.get("exchange_chunks", 1))

    def compress(self, sync_buffer):
        x, xh, lay = self._flat_inputs(sync_buffer)
        q = int(self.quantize_level)
        g = self._gossip(sync_buffer)
        if q == 32 or self.exchange_chunks > 1:
            self._flush_before_pass(g)  # (never deferred on these paths)
        if q != 32 and self.exchange_chunks > 1:
            return self._compress_chunked(sync_buffer, x, xh, lay, q, g)
        sync_buffer.pop("chunked", None)
        self._qsgd_message(sync_buffer, x, xh, lay, gossip=g, pending=self._take_pending)

    def _compress_chunked(self, sync_buffer, x, xh, lay, q, g):
        message, norms, parts = codec.qsgd_chunked_wire(lay.n, q, lay.nseg, self.exchange_chunks, x.device)
        codec.qsgd_norms(x, xhat=xh, seg_off=lay.seg_off, nseg=lay.nseg, gossip=g, out=norms)
        # the norms header leaves first; every range is posted right after its quantize launch,
        # so its transfer (ordered after it on the stream) overlaps the next range's quantize
        head = self._send(sync_buffer, message[:4 * _hdr_words(lay.nseg)])
        seed = self._draw_seed()
        posted = []
        for e0, e1, part in parts:
            codec.qsgd_quantize_range(x, q, norms, e0, e1, part, is_biased=self.is_biased, xhat=xh,
                                      seg_off=lay.seg_off, nseg=lay.nseg, seed=seed)
            posted.append(self._send(sync_buffer, part))
        sync_buffer["chunked"] = (head, [(e0, e1) for e0, e1, _ in parts], posted)
        self._qsgd_keys(sync_buffer, x, message)

    def sync(self, sync_buffer):
        if "chunked" in sync_buffer:  # posted by compress, range by range
            (h_reqs, h_synced), _, posted = sync_buffer["chunked"]
            sync_buffer["sync_reqs"] = h_reqs + [r for p in posted for r in p[0]]
            sync_buffer["synced_message"] = {r: [h_synced[r]] + [p[1][r] for p in posted] for r in h_synced}
            return
        reqs, synced = self._send(sync_buffer, sync_buffer["flatten_updates"].buffer)
        sync_buffer["sync_reqs"] = reqs
        sync_buffer["synced_message"] = synced

    def _uncompress_chunked(self, sync_buffer, neighbor_hat_params, neighbors_info):
        (h_reqs, h_synced), ranges, posted = sync_buffer["chunked"]
        ranks, (weights, self_slot, memory, xhat_self, lay) = self._receive_plan(sync_buffer, neighbor_hat_params,
                                                                                 neighbors_info)
        self.aggregator_fn.complete_wait(h_reqs)
        heads = _received(h_synced, ((r, memory) for r in ranks), codec.qsgd_split, lay.nseg)
        norms = [nm for _, _, (_, nm) in heads]  # the header travels alone: no planes behind it
        for (e0, e1), (reqs, synced) in zip(ranges, posted):
            self.aggregator_fn.complete_wait(reqs)  # this range only: later ones are still in flight
            msgs = [(recover_device(synced[r], device=memory.device), nm) for r, nm in zip(ranks, norms)]
            codec.qsgd_accumulate_range(msgs, weights, self_slot, lay.n, int(self.quantize_level), memory,
                                        e0, e1, xhat_self=xhat_self, is_biased=self.is_biased,
                                        seg_off=lay.seg_off, nseg=lay.nseg)

    def uncompress(self, sync_buffer, neighbor_hat_params, neighbors_info):
        if "chunked" in sync_buffer:
            return self._uncompress_chunked(sync_buffer, neighbor_hat_params, neighbors_info)
        self.aggregator_fn.complete_wait(sync_buffer["sync_reqs"])
        ranks, plan = self._receive_plan(sync_buffer, neighbor_hat_params, neighbors_info)
        weights, self_slot, memory, xhat_self, _ = plan
        msgs = [m for _, _, m in self._qsgd_received(sync_buffer, ((r, memory) for r in ranks))]
        if int(self.quantize_level) == 32:
            for i, (v, w) in enumerate(zip(msgs, weights)):
                if i == self_slot:
                    xhat_self += v
                memory += w * v
            return
        if sync_buffer.get("defer_receive"):  # applied by the next compress's first pass
            return self._defer(msgs, *plan)
        self._apply(msgs, *plan)

    def _apply(self, parts, weights, self_slot, memory, xhat_self, lay):
        codec.qsgd_accumulate(parts, weights, self_slot, lay.n, int(self.quantize_level), memory,
                              xhat_self=xhat_self, is_biased=self.is_biased, seg_off=lay.seg_off, nseg=lay.nseg)


class _Reassembled(_LazyDict):
    """{rank: [norms | words] message} of a chunked sign exchange over an aggregator without
    `out=`: each neighbour's message is concatenated from its received ranges on first
    access, i.e. after uncompress has waited for every request."""

    def __init__(self, rank, message, head, parts):
        super().__init__()
        self._src = {r: (head[r], [p[r] for p in parts]) for r in head if r != rank}
        self[rank] = message
        for r in self._src:
            dict.__setitem__(self, r, None)

    def __getitem__(self, r):
        v = dict.__getitem__(self, r)
        if v is None:
            h, ps = self._src[r]
            v = torch.cat([h] + ps)
            dict.__setitem__(self, r, v)
        return v


class _LazyMap(_LazyDict):
    """{rank: fn(src[rank])}, evaluated on access."""

    def __init__(self, src, fn):
        super().__init__((r, None) for r in src.keys())
        self._src, self._fn = src, fn

    def __getitem__(self, r):
        return self._fn(self._src[r])


class CHOCOSignCompressor(_CHOCOBase):
    """sign + per-tensor L1 norm  (parallel_choco_v.py:436-558).

    `exchange_chunks=C` (> 1, every rank alike) pipelines the send with the pack: the
    words are packed in C column ranges and each range's words are posted as soon as its
    pack is queued (its transfer overlaps the next range's pack); the norms header, complete
    only after the last range, leaves last.  Every range of the (32, N') layout touches
    every row's segments, so the receiver decodes after the whole message, as with C = 1
    (include/choco_codec.h "Chunked sign pack").  Neighbours receive straight into one
    message per rank, so the wire, `synced_message` and the decode are those of C = 1."""

    placeholder_key = "flatten_directions"

    def __init__(self, *args, **kargs):
        super().__init__(*args, **kargs)
        self.exchange_chunks = int(self.kargs.get("exchange_chunks", 1))

    def compress(self, sync_buffer):
        x, xh, lay = self._flat_inputs(sync_buffer)
        g = self._gossip(sync_buffer)
        sync_buffer.pop("chunked", None)
        if self.exchange_chunks == 1:
            self._sign_message(sync_buffer, x, xh, lay, gossip=g, pending=self._take_pending)
            return
        message, (signs, norms) = codec.sign_wire(lay.n, lay.nseg, x.device)  # written in place by the kernels
        self._flush_before_pass(g)  # (never deferred on this path)
        sync_buffer["chunked"] = self._pack_and_post(sync_buffer, x, xh, lay, g, message, signs, norms)
        self._sign_keys(sync_buffer, message, signs, norms, lay)

    def _agg_takes_out(self):
        """Whether the aggregator's _agg accepts `out=` (this package's DecentralizedAggregation
        does; the reference's, communication.py:246, does not)."""
        try:
            ps = inspect.signature(self.aggregator_fn._agg).parameters
        except (TypeError, ValueError):
            return False
        return "out" in ps or any(p.kind == p.VAR_KEYWORD for p in ps.values())

    def _pack_and_post(self, sync_buffer, x, xh, lay, g, message, signs, norms):
        try:
            return self._pack_and_post_ranges(sync_buffer, x, xh, lay, g, message, signs, norms)
        except BaseException:
            # the per-segment L1 sums of the ranges packed so far stay in the stream's
            # accumulator workspace until the `finish` range clears them: drop it, so the next
            # sign / QSGD call does not add stale sums into its norms
            codec.drop_workspace(x.device, "acc")
            raise

    def _pack_and_post_ranges(self, sync_buffer, x, xh, lay, g, message, signs, norms):
        # the ranges are the unit that travels here: a range of the message's words
        # (codec.sign_chunks counts from the end of the header), and the header, sent last
        hw = _hdr_words(lay.nseg)
        ranges = codec.sign_chunks(lay.n, self.exchange_chunks)
        if not self._agg_takes_out():
            # the reference's aggregator: every range travels as a message of its own (same
            # posting order); uncompress re-assembles each neighbour's [norms | words]
            parts, reqs = [], []
            for i, (w0, w1) in enumerate(ranges):
                codec.sign_compress_range(x, w0, w1, i == len(ranges) - 1, xhat=xh, seg_off=lay.seg_off,
                                          nseg=lay.nseg, gossip=g, out=(signs, norms))
                r, synced = self._send(sync_buffer, message[hw + w0:hw + w1])
                reqs += r
                parts.append(synced)
            r, head = self._send(sync_buffer, message[:hw])
            return reqs + r, _Reassembled(self.aggregator_fn.rank, message, head, parts)
        peers = [r for r in self.aggregator_fn.neighbor_ranks]
        host = self.comm_device == "cpu"
        recv = {r: torch.empty(message.shape, dtype=message.dtype, device="cpu" if host else message.device,
                               pin_memory=host) for r in peers}
        reqs = []
        for i, (w0, w1) in enumerate(ranges):
            codec.sign_compress_range(x, w0, w1, i == len(ranges) - 1, xhat=xh, seg_off=lay.seg_off,
                                      nseg=lay.nseg, gossip=g, out=(signs, norms))
            r, _ = self._send(sync_buffer, message[hw + w0:hw + w1],
                              out={p: recv[p][hw + w0:hw + w1] for p in peers})
            reqs += r
        r, _ = self._send(sync_buffer, message[:hw], out={p: recv[p][:hw] for p in peers})
        recv[self.aggregator_fn.rank] = message
        return reqs + r, recv

    def sync(self, sync_buffer):
        if "chunked" in sync_buffer:  # posted by compress, range by range
            reqs, synced = sync_buffer["chunked"]
        else:
            reqs, synced = self._send(sync_buffer, sync_buffer["sign_message"])  # [norms | signs]
        sync_buffer["sync_reqs_1"] = reqs
        sync_buffer["sync_reqs_2"] = []
        if isinstance(synced, _Reassembled):  # assembled after uncompress's wait, not now
            nseg = sync_buffer["flatten_norms"].buffer.numel()
            sync_buffer["synced_message"] = synced
            sync_buffer["synced_flatten_norms"] = _LazyMap(synced, lambda m: codec.sign_split(m, nseg)[1])
            sync_buffer["synced_signs"] = _LazyMap(synced, lambda m: codec.sign_split(m, nseg)[0])
        else:
            self._sign_synced(sync_buffer, synced)

    def uncompress(self, sync_buffer, neighbor_hat_params, neighbors_info):
        self.aggregator_fn.complete_wait(sync_buffer["sync_reqs_1"])
        self.aggregator_fn.complete_wait(sync_buffer["sync_reqs_2"])
        ranks, plan = self._receive_plan(sync_buffer, neighbor_hat_params, neighbors_info)
        memory = plan[2]
        parts = [m for _, _, m in self._sign_received(sync_buffer, ((r, memory) for r in ranks))]
        if sync_buffer.get("defer_receive") and "chunked" not in sync_buffer:  # the next compress applies them
            return self._defer(parts, *plan)
        self._apply(parts, *plan)

    def _apply(self, parts, weights, self_slot, memory, xhat_self, lay):
        codec.sign_accumulate(parts, weights, self_slot, lay.n, memory, xhat_self=xhat_self, seg_off=lay.seg_off,
                              nseg=lay.nseg)


class CHOCOCompressor(_Facade):
    sparsification, quantization, sign = CHOCOSparsificationCompressor, CHOCOQuantizationCompressor, CHOCOSignCompressor

    def pipeline(self, *args, **kargs):
        return self.compressor_fn.pipeline(*args, **kargs)

    def flush_receive(self):
        return self.compressor_fn.flush_receive()
