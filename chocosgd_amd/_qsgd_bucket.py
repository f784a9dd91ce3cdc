"""The Python side of the bucketed max-norm QSGD entry points (csrc/qsgd_bucket.hip;
include/choco_codec.h "bucketed QSGD").  codec.py re-exports these as `codec.qsgd_bucket_*`; their
stream-ordering case stands in tests/test_gpu_qsgd_bucket.py."""
import torch

from . import _lib
from . import codec as _c

QSGD_BUCKETS = (128, 256, 512, 1024, 2048)


def qsgd_bucket_packed_bytes(n, q, bucket=512):
    """Bytes of one bucketed message [scales (16-B padded) | level plane | sign plane]."""
    nbytes = int(_c.lib().choco_qsgd_bucket_packed_bytes(int(n), int(q), int(bucket)))
    if nbytes == 0:
        raise RuntimeError(f"bucketed QSGD takes n >= 1, q in [1, 16] and a bucket of {QSGD_BUCKETS}; got n={n}, "
                           f"q={q}, bucket={bucket}")
    return nbytes


def qsgd_bucket_wire(n, q, bucket, dev):
    """One bucketed QSGD message (uint8); the kernels write every byte of it, padding included."""
    return torch.empty(qsgd_bucket_packed_bytes(n, q, bucket), dtype=torch.uint8, device=dev)


def qsgd_bucket_split(message, n, q, bucket):
    """A bucketed message taken apart: (scales f32[nb], level plane, sign plane), views of it."""
    nb = -(-int(n) // int(bucket))
    sb = (4 * nb + 15) // 16 * 16
    lb = sb + (_c.qsgd_packed_bytes(n, q) - (-(-int(n) // 8) + 15) // 16 * 16)
    return message[:sb].view(torch.float32)[:nb], message[sb:lb], message[lb:]


def _bucket_msgs(messages, weights, self_slot, nbytes):
    """The C tables of a bucketed multi-message call: (messages**, weights*, count, slot, keep-alive)."""
    if len(messages) != len(weights) or not 1 <= len(messages) <= _c.MAX_FUSED_MSGS:
        raise RuntimeError(f"one weight per message, 1 to {_c.MAX_FUSED_MSGS} messages")
    for m in messages:
        _c._require(m, torch.uint8, "message")
        if m.numel() != nbytes:
            raise RuntimeError(f"bucketed QSGD message must hold {nbytes} bytes, got {m.numel()}")
    pp, keep1 = _lib.ptr_array([m.data_ptr() for m in messages])
    ww, keep2 = _lib.f32_array([float(w) for w in weights])
    return pp, ww, len(messages), int(self_slot), (keep1, keep2)


def qsgd_bucket_compress(x, q, bucket=512, is_biased=False, xhat=None, u_in=None, seed=0, offset=0,
                         want_dense=False, gossip=None, out=None):
    """Bucketed max-norm QSGD in one pass (include/choco_codec.h "bucketed QSGD").  Returns
    (message uint8, dense f32[n] or None).  `gossip=(memory, gamma)` applies the consensus step
    to x first, in the same pass; `out=` is a caller's qsgd_bucket_wire buffer."""
    _c._require(x, torch.float32, "x")
    n, dev = x.numel(), x.device
    for t, nm in ((xhat, "xhat"), (u_in, "u_in")):
        if t is not None:
            _c._require(t, torch.float32, nm)
            if t.numel() != n:
                raise RuntimeError(f"{nm} must have one value per element")
    message = out if out is not None else qsgd_bucket_wire(n, q, bucket, dev)
    _c._require(message, torch.uint8, "out")
    if message.numel() != qsgd_bucket_packed_bytes(n, q, bucket) or message.device != dev:
        raise RuntimeError(f"out must hold qsgd_bucket_packed_bytes(n, q, bucket) bytes on {dev}")
    dense = torch.empty(n, dtype=torch.float32, device=dev) if want_dense else None
    tail = (int(q), int(bucket), 1 if is_biased else 0, _c._ptr(u_in), int(seed) & (2**64 - 1),
            int(offset) & (2**64 - 1), _c._ptr(message), _c._ptr(dense), _c._stream(dev))
    g = _c._gossip(gossip, x, xhat)
    if g is not None:
        _lib.check(_c.lib().choco_gossip_qsgd_bucket_compress(_c._ptr(x), _c._ptr(g[0]), _c._ptr(xhat), g[1], n,
                                                              *tail), "choco_gossip_qsgd_bucket_compress")
    else:
        _lib.check(_c.lib().choco_qsgd_bucket_compress(_c._ptr(x), _c._ptr(xhat), n, *tail),
                   "choco_qsgd_bucket_compress")
    return message, dense


def qsgd_bucket_decode(message, n, q, bucket=512, is_biased=False):
    _c._require(message, torch.uint8, "message")
    if message.numel() != qsgd_bucket_packed_bytes(n, q, bucket):
        raise RuntimeError("message must hold qsgd_bucket_packed_bytes(n, q, bucket) bytes")
    out = torch.empty(n, dtype=torch.float32, device=message.device)
    _lib.check(_c.lib().choco_qsgd_bucket_decode(_c._ptr(message), int(n), int(q), int(bucket),
                                                 1 if is_biased else 0, _c._ptr(out), _c._stream(message.device)),
               "choco_qsgd_bucket_decode")
    return out


def qsgd_bucket_accumulate(messages, weights, self_slot, n, q, memory, bucket=512, xhat_self=None, is_biased=False):
    """messages: bucketed messages applied in order; any count (fused chunks of MAX_FUSED_MSGS)."""
    _c._require(memory, torch.float32, "memory")
    _c._check_layout(memory, xhat_self, n, None, 1)
    nbytes = qsgd_bucket_packed_bytes(n, q, bucket)
    for c0 in range(0, len(messages), _c.MAX_FUSED_MSGS):
        part = messages[c0:c0 + _c.MAX_FUSED_MSGS]
        slot = self_slot - c0 if c0 <= self_slot < c0 + len(part) else -1
        pp, ww, m, slot, _keep = _bucket_msgs(part, weights[c0:c0 + len(part)], slot, nbytes)
        _lib.check(_c.lib().choco_qsgd_bucket_decompress_accumulate(
            pp, ww, m, slot, int(n), int(q), int(bucket), 1 if is_biased else 0,
            _c._ptr(xhat_self if slot >= 0 else None), _c._ptr(memory), _c._stream(memory.device)),
            "choco_qsgd_bucket_decompress_accumulate")


def qsgd_bucket_recv_gossip_compress(messages, weights, self_slot, x, memory, xhat, gamma, q, bucket=512,
                                     is_biased=False, u_in=None, seed=0, offset=0, out=None):
    """The whole CHOCO step in one kernel (choco_qsgd_bucket_recv_gossip_compress): the previous
    step's messages into x_hat (self_slot) and memory in order, x += gamma (memory - x_hat), then
    this step's message of x - x_hat, returned or written to `out` (no input message's buffer).
    More than 8 messages: the leading ones are applied by qsgd_bucket_accumulate first."""
    for t, nm in ((x, "x"), (xhat, "xhat"), (memory, "memory")):
        _c._require(t, torch.float32, nm)
    n, dev = x.numel(), x.device
    _c._check_layout(memory, xhat, n, None, 1)
    if u_in is not None:
        _c._require(u_in, torch.float32, "u_in")
        if u_in.numel() != n:
            raise RuntimeError("u_in must have one uniform per element")
    nbytes = qsgd_bucket_packed_bytes(n, q, bucket)
    message = out if out is not None else qsgd_bucket_wire(n, q, bucket, dev)
    _c._require(message, torch.uint8, "out")
    if message.numel() != nbytes or message.device != dev:
        raise RuntimeError(f"out must hold qsgd_bucket_packed_bytes(n, q, bucket) bytes on {dev}")
    head = max(0, len(messages) - _c.MAX_FUSED_MSGS)
    if head > 0:
        qsgd_bucket_accumulate(messages[:head], weights[:head], self_slot, n, q, memory, bucket=bucket,
                               xhat_self=xhat if 0 <= self_slot < head else None, is_biased=is_biased)
    pp, ww, m, slot, _keep = _bucket_msgs(messages[head:], weights[head:], max(self_slot - head, -1), nbytes)
    _lib.check(_c.lib().choco_qsgd_bucket_recv_gossip_compress(
        pp, ww, m, slot, _c._ptr(x), _c._ptr(memory), _c._ptr(xhat), float(gamma), n, int(q), int(bucket),
        1 if is_biased else 0, _c._ptr(u_in), int(seed) & (2**64 - 1), int(offset) & (2**64 - 1), _c._ptr(message),
        _c._stream(dev)), "choco_qsgd_bucket_recv_gossip_compress")
    return message
