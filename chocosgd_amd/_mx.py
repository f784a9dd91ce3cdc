"""The Python side of the MX (block-scaled FP4 / FP8) entry points (csrc/mx.hip;
include/choco_codec.h "MX wire").  codec.py re-exports these as `codec.mx_*`; their
stream-ordering case stands in tests/test_gpu_mx.py."""
import torch

from . import _lib
from . import codec as _c

MX_LEVELS = (4, 8)  # quantize_level 4: E2M1, 8: E4M3
MX_BLOCK = 32
_U64 = 2**64 - 1


def mx_packed_bytes(n, q):
    """Bytes of one MX message [scale bytes (16-B padded) | codes (16-B padded)]."""
    nbytes = int(_c.lib().choco_mx_packed_bytes(int(n), int(q)))
    if nbytes == 0:
        raise RuntimeError(f"the MX wire takes n >= 1 and quantize_level 4 (E2M1) or 8 (E4M3); got n={n}, "
                           f"quantize_level={q}")
    return nbytes


def mx_wire(n, q, dev):
    """One MX message (uint8); the kernels write every byte of it, padding included."""
    return torch.empty(mx_packed_bytes(n, q), dtype=torch.uint8, device=dev)


def mx_split(message, n, q):
    """An MX message taken apart: (scale bytes u8[ceil(n / 32)], code bytes u8[ceil(n q / 8)]), views of it."""
    nb = -(-int(n) // MX_BLOCK)
    sb = (nb + 15) // 16 * 16
    return message[:nb], message[sb:sb + (int(n) * int(q) + 7) // 8]


def _mx_msgs(messages, weights, self_slot, nbytes):
    """The C tables of a multi-message call: (messages**, weights*, count, slot, keep-alive)."""
    if len(messages) != len(weights) or not 1 <= len(messages) <= _c.MAX_FUSED_MSGS:
        raise RuntimeError(f"one weight per message, 1 to {_c.MAX_FUSED_MSGS} messages")
    for m in messages:
        _c._require(m, torch.uint8, "message")
        if m.numel() != nbytes:
            raise RuntimeError(f"MX message must hold {nbytes} bytes, got {m.numel()}")
    pp, keep1 = _lib.ptr_array([m.data_ptr() for m in messages])
    ww, keep2 = _lib.f32_array([float(w) for w in weights])
    return pp, ww, len(messages), int(self_slot), (keep1, keep2)


def _out_wire(out, n, q, dev):
    message = out if out is not None else mx_wire(n, q, dev)
    _c._require(message, torch.uint8, "out")
    if message.numel() != mx_packed_bytes(n, q) or message.device != dev:
        raise RuntimeError(f"out must hold mx_packed_bytes(n, q) bytes on {dev}")
    return message


def mx_compress(x, q, is_biased=False, xhat=None, seed=0, offset=0, want_dense=False, gossip=None, out=None):
    """The MX message of x - xhat in one pass.  is_biased=False rounds stochastically (unbiased; the
    message is a function of (d, seed, offset)), True to nearest even.  Returns (message uint8, dense
    f32[n] or None).  `gossip=(memory, gamma)` applies the consensus step to x first, in the same pass;
    `out=` is a caller's mx_wire buffer."""
    _c._require(x, torch.float32, "x")
    n, dev = x.numel(), x.device
    if xhat is not None:
        _c._require(xhat, torch.float32, "xhat")
        if xhat.numel() != n:
            raise RuntimeError("xhat must have one value per element")
    message = _out_wire(out, n, q, dev)
    dense = torch.empty(n, dtype=torch.float32, device=dev) if want_dense else None
    tail = (int(q), 0 if is_biased else 1, int(seed) & _U64, int(offset) & _U64, _c._ptr(message), _c._ptr(dense),
            _c._stream(dev))
    g = _c._gossip(gossip, x, xhat)
    if g is not None:
        _lib.check(_c.lib().choco_gossip_mx_compress(_c._ptr(x), _c._ptr(g[0]), _c._ptr(xhat), g[1], n, *tail),
                   "choco_gossip_mx_compress")
    else:
        _lib.check(_c.lib().choco_mx_compress(_c._ptr(x), _c._ptr(xhat), n, *tail), "choco_mx_compress")
    return message, dense


def mx_decode(message, n, q):
    _c._require(message, torch.uint8, "message")
    if message.numel() != mx_packed_bytes(n, q):
        raise RuntimeError("message must hold mx_packed_bytes(n, q) bytes")
    out = torch.empty(n, dtype=torch.float32, device=message.device)
    _lib.check(_c.lib().choco_mx_decode(_c._ptr(message), int(n), int(q), _c._ptr(out), _c._stream(message.device)),
               "choco_mx_decode")
    return out


def mx_accumulate(messages, weights, self_slot, n, q, memory, xhat_self=None):
    """messages: MX messages applied in order; any count (fused chunks of MAX_FUSED_MSGS)."""
    _c._require(memory, torch.float32, "memory")
    _c._check_layout(memory, xhat_self, n, None, 1)
    nbytes = mx_packed_bytes(n, q)
    for c0 in range(0, len(messages), _c.MAX_FUSED_MSGS):
        part = messages[c0:c0 + _c.MAX_FUSED_MSGS]
        slot = self_slot - c0 if c0 <= self_slot < c0 + len(part) else -1
        pp, ww, m, slot, _keep = _mx_msgs(part, weights[c0:c0 + len(part)], slot, nbytes)
        _lib.check(_c.lib().choco_mx_decompress_accumulate(
            pp, ww, m, slot, int(n), int(q), _c._ptr(xhat_self if slot >= 0 else None), _c._ptr(memory),
            _c._stream(memory.device)), "choco_mx_decompress_accumulate")


def mx_recv_gossip_compress(messages, weights, self_slot, x, memory, xhat, gamma, q, is_biased=False, seed=0,
                            offset=0, out=None):
    """The whole CHOCO step in one kernel (choco_mx_recv_gossip_compress): the previous step's messages
    into x_hat (self_slot) and memory in order, x += gamma (memory - x_hat), then this step's message of
    x - x_hat, returned or written to `out` (no input message's buffer).  More than 8 messages: the
    leading ones are applied by mx_accumulate first."""
    for t, nm in ((x, "x"), (xhat, "xhat"), (memory, "memory")):
        _c._require(t, torch.float32, nm)
    n, dev = x.numel(), x.device
    _c._check_layout(memory, xhat, n, None, 1)
    message = _out_wire(out, n, q, dev)
    head = max(0, len(messages) - _c.MAX_FUSED_MSGS)
    if head > 0:
        mx_accumulate(messages[:head], weights[:head], self_slot, n, q, memory,
                      xhat_self=xhat if 0 <= self_slot < head else None)
    pp, ww, m, slot, _keep = _mx_msgs(messages[head:], weights[head:], max(self_slot - head, -1), message.numel())
    _lib.check(_c.lib().choco_mx_recv_gossip_compress(
        pp, ww, m, slot, _c._ptr(x), _c._ptr(memory), _c._ptr(xhat), float(gamma), n, int(q), 0 if is_biased else 1,
        int(seed) & _U64, int(offset) & _U64, _c._ptr(message), _c._stream(dev)), "choco_mx_recv_gossip_compress")
    return message
