"""The drop-in compressors' contract, case by case (tests/test_gpu_dropin_contract.py asserts
what this module produces against tests/golden/dropin_contract.json, which
tests/golden/gen_dropin_contract.py recorded with it).

Every case drives one family (CHOCO, DCD, ECD, DeepSqueeze, EF-sign, DGCCodec) through its
three calls on three in-process ranks: ranks 0 and 2 compress and send first into an
aggregator that keeps what they send, then rank 1 runs against an aggregator that hands those
messages back beside its own.  Recorded for rank 1, after each of its calls: the
`sync_buffer` keys that call added or changed (and those it removed; the caller's own input
keys appear only where a call changes them), each with a descriptor
(type; dtype, shape and device type of a tensor; a TensorBuffer's buffer and `_tensors_sizes`;
containers entry by entry; scalars by value) and, for every tensor, `wire` = its byte offset
into the storage of the wire message this rank built (None: not a view of it) and, inside a
per-rank container, `msg` = the same against `synced_message[rank]`.  Recorded for the whole
case: the `codec.*` calls made from outside codec.py in order, arguments by parameter name
(those that have their default left out) with tensors reduced to dtype and numel; every
aggregator call (the keywords given, the message's dtype and numel, whether `out=` came) and
every `complete_wait`; one draw from torch's generator after the case (it pins the number of
`_draw_seed()` draws); sha256 of every message rank 1 sent and of every tensor the case
updates.

Inputs are seeded integers / 64 with |x| <= 4 (numpy's generator: torch's is the one being
counted), so every fp64 partial sum of |x| or x^2 is exact in any order (n * 4 * 64 < 2^24,
n * 16 * 4096 < 2^53) and the norms, and with them the QSGD levels, do not depend on the order
of the kernels' atomics.  Weights and step sizes are powers of two.

LENS: 7 tensors pad the norms header 7 -> 8 words, one tensor has a single element, n = 3161
is no multiple of 32 (the sign tail word) or of 8 (the QSGD plane tail).  LENS_CHUNKED adds
40,000 elements: more than one 1024-word sign range and more than one 8192-element QSGD range,
for the `exchange_chunks=2` cases only.

Which codec functions are traced is part of the recorded file (`traced`: the public functions
of codec.py when it was recorded, less `lib` and `wire_header_words`); functions codec.py gains
later -- the wire format's split functions are such -- are views of a message, launch nothing
and are not traced.
"""
import functools
import hashlib
import inspect
import sys
import types

import numpy as np
import torch

DEV = "cuda"
LENS = [5, 1, 64, 33, 1000, 7, 2051]
LENS_CHUNKED = LENS + [40000]
SELF, RANKS = 1, (0, 2, 1)  # rank 1 runs last, against what 0 and 2 sent
WEIGHTS = {0: 0.25, 1: 0.5, 2: 0.25}
GAMMA = 0.5
SEED0 = 7000
UNTRACED = ("lib", "wire_header_words")
_UNSET = "<unset>"

OPS = {"top_k": dict(comm_op="compress_top_k"), "random_k": dict(comm_op="compress_random_k"),
       "qsgd4": dict(comm_op="quantize_qsgd", quantize_level=4),
       "qsgd32": dict(comm_op="quantize_qsgd", quantize_level=32), "sign": dict(comm_op="sign")}


def traced_names():
    from chocosgd_amd import codec
    return sorted(n for n, f in vars(codec).items() if isinstance(f, types.FunctionType)
                  and f.__module__ == codec.__name__ and not n.startswith("_") and n not in UNTRACED)


# ----------------------------------------------------------------------------- inputs, hashes
def ints(seed, n):
    a = np.random.RandomState(seed).randint(-256, 257, size=n).astype(np.float32) / 64
    return torch.from_numpy(a).to(DEV)


def tb(flat, lens):
    from chocosgd_amd.tensor_buffer import TensorBuffer
    return TensorBuffer.from_flat(flat, [(m,) for m in lens])


def shapes(lens):
    return [(torch.Size([m]), m) for m in lens]


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


# ----------------------------------------------------------------------------- descriptors
def _store(t):
    return t.untyped_storage().data_ptr() if isinstance(t, torch.Tensor) and t.numel() else None


def _off(t, base):
    return t.data_ptr() - base if base is not None and _store(t) == base else None


def describe(v, wire, msgs=None, rank=None, lazy=True):
    """msgs: {rank: storage of synced_message[rank]}; rank: the per-rank entry v sits in."""
    from chocosgd_amd.tensor_buffer import TensorBuffer
    name = type(v).__name__
    if isinstance(v, torch.Tensor):
        d = "{}{}@{} wire={}".format(str(v.dtype).replace("torch.", ""), list(v.shape), v.device.type,
                                     _off(v, wire))
        if rank is not None and msgs and rank in msgs:
            d += " msg={}".format(_off(v, msgs[rank]))
        return d
    if isinstance(v, TensorBuffer):
        sizes = ",".join("x".join(str(d) for d in s) or "()" for s in v._tensors_sizes)
        return "TensorBuffer({}) sizes={}".format(describe(v.buffer, wire, msgs, rank), sizes)
    if isinstance(v, dict):
        if type(v) is not dict and not lazy:  # assembled on access: looked into after uncompress's wait only
            return {name: [repr(k) for k in v.keys()]}
        return {name: {repr(k): describe(v[k], wire, msgs, k if rank is None else rank, lazy) for k in v.keys()}}
    if isinstance(v, (list, tuple)) and not isinstance(v, torch.Size):
        per_rank = rank is None and len(v) == len(RANKS) and all(isinstance(e, torch.Tensor) for e in v)
        return {name: [describe(e, wire, msgs, i if per_rank else rank, lazy) for i, e in enumerate(v)]}
    if v is None or isinstance(v, (bool, int, float, str, torch.Size)):
        return "{} {!r}".format(name, v)
    return name


def describe_buffer(sb, lazy=True):
    """{key: descriptor} of a sync_buffer (sorted by the JSON writer)."""
    wire = None
    for key in ("wire_message", "sign_message"):
        if isinstance(sb.get(key), torch.Tensor):
            wire = _store(sb[key])
    if wire is None and sb.get("flatten_updates") is not None:
        wire = _store(sb["flatten_updates"].buffer)
    msgs = None
    synced = sb.get("synced_message")
    if isinstance(synced, dict) and (lazy or type(synced) is dict):
        msgs = {r: _store(synced[r]) for r in synced.keys() if isinstance(synced[r], torch.Tensor)}
    elif isinstance(synced, list):
        msgs = {r: _store(m) for r, m in enumerate(synced)}
    return {str(k): describe(v, wire, msgs, None, lazy) for k, v in sb.items()}


def changes(before, after):
    """What a call did to the keys: [{key: descriptor} of the new and the changed ones, [keys gone]]."""
    return [{k: d for k, d in sorted(after.items()) if before.get(k) != d}, sorted(set(before) - set(after))]


# ----------------------------------------------------------------------------- traces
def _plain(v):
    """An argument as the trace shows it: a tensor as dtype[numel], an object as its type's name."""
    if isinstance(v, torch.Tensor):
        return "{}[{}]".format(str(v.dtype).replace("torch.", ""), v.numel())
    if isinstance(v, (list, tuple)):
        return "[{}]".format(", ".join(_plain(e) for e in v))
    if isinstance(v, dict):
        return "{{{}}}".format(", ".join("{!r}: {}".format(k, _plain(e)) for k, e in v.items()))
    if v is None or isinstance(v, (bool, int, float, str)):
        return repr(v)
    return type(v).__name__


class Trace:
    """The codec calls that come from outside codec.py, and the aggregator calls."""

    def __init__(self, monkeypatch, names):
        from chocosgd_amd import codec
        self.codec, self.agg = [], []
        for name in names:
            monkeypatch.setattr(codec, name, self._wrap(name, getattr(codec, name), codec.__name__))

    def _wrap(self, name, fn, module):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def call(*a, **kw):
            if sys._getframe(1).f_globals.get("__name__") != module:
                # without the arguments that have their default: passing it explicitly is the same call
                given = {k: _plain(v) for k, v in sig.bind(*a, **kw).arguments.items()}
                args = ", ".join("{}={}".format(k, v) for k, v in sorted(given.items())
                                 if v != _plain(sig.parameters[k].default))
                self.codec.append("{}({})".format(name, args))
            return fn(*a, **kw)
        return call


class Loop:
    """Rank `rank` of three, in process.  Without `peers` it keeps what is sent and hands a copy
    back in the neighbours' places; with `peers` = {rank: [message of call 0, 1, ...]} it hands
    those back.  The signature is the reference's (no `out=`); LoopOut's takes it."""

    def __init__(self, rank, trace, peers=None):
        self.rank, self.trace, self.peers = rank, trace, peers
        self.neighbor_ranks = [r for r in sorted(RANKS) if r != rank]
        self.sent = []

    def _peer(self, r, data):
        c = len(self.sent) - 1
        return data.clone() if self.peers is None else self.peers[r][c].to(data.device)

    def _exchange(self, data, given, out=None):
        given_ = ", ".join("{}={!r}".format(k, v) for k, v in given.items() if v is not _UNSET)
        self.trace.agg.append("_agg({}[{}], {}{})".format(str(data.dtype).replace("torch.", ""), data.numel(), given_,
                                                         ", out=..." if out is not None else ""))
        self.sent.append(data.clone())
        if out is not None:
            for r in self.neighbor_ranks:
                out[r].copy_(self._peer(r, data))
        local = {r: data if r == self.rank else (out[r] if out is not None else self._peer(r, data))
                 for r in sorted(RANKS)}
        scheme = given["communication_scheme"]
        if scheme == "all_gather":
            return [local[r] for r in sorted(RANKS)]
        if scheme == "all_reduce":
            return local[0] + local[1] + local[2]
        if given["force_wait"] is False:
            return [len(self.sent) - 1], local
        return local

    def _agg(self, data, op=_UNSET, force_wait=_UNSET, communication_scheme=_UNSET, async_op=_UNSET):
        return self._exchange(data, dict(op=op, force_wait=force_wait, communication_scheme=communication_scheme,
                                         async_op=async_op))

    def complete_wait(self, reqs):
        self.trace.agg.append("complete_wait({})".format(list(reqs)))


class LoopOut(Loop):
    def _agg(self, data, op=_UNSET, force_wait=_UNSET, communication_scheme=_UNSET, async_op=_UNSET, out=None):
        return self._exchange(data, dict(op=op, force_wait=force_wait, communication_scheme=communication_scheme,
                                         async_op=async_op), out)


def _nine(agg, op, **kw):
    args = dict(aggregator=agg, comm_op="sign", comm_device="gpu", compress_ratio=0.9, quantize_level=4,
                is_biased=False, backend="nccl", use_ipc=False)
    args.update(OPS[op])
    args.update(kw)
    return args


class Case:
    """One case's record; `ranks()` yields (rank, aggregator) with rank 1 last."""

    def __init__(self, monkeypatch, names, seed, agg_cls=Loop):
        self.trace = Trace(monkeypatch, names)
        self.seed, self.agg_cls = seed, agg_cls
        self.calls, self.hashes, self._keys = [], {}, {}

    def ranks(self):
        sent = {}
        for r in RANKS:
            agg = self.agg_cls(r, self.trace, peers=sent if r == SELF else None)
            torch.manual_seed(SEED0 + 10 * self.seed + r)
            yield r, agg
            sent[r] = agg.sent
        for i, m in enumerate(agg.sent):
            self.hashes[f"sent{i}"] = sha(m)

    def ints(self, r, what, n):
        return ints(1000 * self.seed + 10 * what + r, n)

    def given(self, sb):
        """The caller's own keys, before the first call: not part of what the calls write."""
        self._keys = describe_buffer(sb)

    def after(self, call, sb, lazy=True):
        keys = describe_buffer(sb, lazy)
        self.calls.append([call] + changes(self._keys, keys))
        self._keys = keys

    def state(self, **tensors):
        for k, t in tensors.items():
            self.hashes[k] = sha(t)

    def result(self):
        torch.cuda.synchronize()
        return {"calls": self.calls, "codec": self.trace.codec, "agg": self.trace.agg,
                "rng": int(torch.randint(0, 2**62, (1,)).item()), "hashes": self.hashes}


# ----------------------------------------------------------------------------- the families
def choco(case, op, gossip=False, chunks=1, steps=1):
    from chocosgd_amd.parallel_choco import CHOCOCompressor
    lens = LENS_CHUNKED if chunks > 1 else LENS
    n = sum(lens)
    kw = dict(exchange_chunks=chunks) if chunks > 1 else {}
    for r, agg in case.ranks():
        comp = CHOCOCompressor(**_nine(agg, op, **kw))
        x, xh, mem = (tb(case.ints(r, w, n), lens) for w in range(3))
        sb = {"original_shapes": shapes(lens), "flatten_params": x, "flatten_hat_params": xh}
        if gossip:
            sb["gossip"] = (mem.buffer, GAMMA)
        nhp = {SELF: xh, "memory": mem}
        if steps > 1:
            sb["defer_receive"] = True
        if r == SELF:
            case.given(sb)
        for step in range(steps):
            tag = f"step{step}." if steps > 1 else ""
            comp.compress(sb)
            if r == SELF:
                case.after(tag + "compress", sb)
            comp.sync(sb)
            if r != SELF:
                continue  # the neighbours only send
            case.after(tag + "sync", sb, lazy=False)
            comp.uncompress(sb, nhp, WEIGHTS)
            case.after(tag + "uncompress", sb)
        if r == SELF:
            if steps > 1:
                case.state(x_deferred=x.buffer, xhat_deferred=xh.buffer, memory_deferred=mem.buffer)
                comp.flush_receive()
            case.state(x=x.buffer, xhat=xh.buffer, memory=mem.buffer)


def dcd(case, op):
    from chocosgd_amd.dcd import DCDCompressor
    n = sum(LENS)
    for r, agg in case.ranks():
        comp = DCDCompressor(**_nine(agg, op))
        half, x = (tb(case.ints(r, w, n), LENS) for w in range(2))
        sb = {"original_shapes": shapes(LENS), "flatten_half_params": half, "flatten_params": x}
        if r == SELF:
            case.given(sb)
        comp.compress(sb)
        if r == SELF:
            case.after("compress", sb)
        comp.sync(sb)
        if r == SELF:
            case.after("sync", sb)
            nhp = {q: tb(case.ints(q, 5, n), LENS) for q in sorted(RANKS)}
            comp.uncompress(sb, nhp)
            case.after("uncompress", sb)
            case.state(half=half.buffer, x=x.buffer, **{f"replica{q}": h.buffer for q, h in nhp.items()})


def ecd(case, op):
    from chocosgd_amd.ecd import ECDCompressor
    n = sum(LENS)
    for r, agg in case.ranks():
        comp = ECDCompressor(**_nine(agg, op))
        x = tb(case.ints(r, 0, n), LENS)
        sb = {"original_shapes": shapes(LENS), "flatten_updated_params": x}
        if r == SELF:
            case.given(sb)
        comp.compress(sb)
        if r == SELF:
            case.after("compress", sb)
        comp.sync(sb)
        if r == SELF:
            case.after("sync", sb)
            nhp = {q: tb(case.ints(q, 5, n), LENS) for q in sorted(RANKS)}
            comp.uncompress(sb, nhp, 3)
            case.after("uncompress", sb)
            case.state(x=x.buffer, **{f"replica{q}": h.buffer for q, h in nhp.items()})


def deep_squeeze(case, op, residual=False):
    from chocosgd_amd.deep_squeeze import DeepSqueezeCompressor
    n = sum(LENS)
    for r, agg in case.ranks():
        comp = DeepSqueezeCompressor(rank=r, consensus_stepsize=GAMMA, **_nine(agg, op))
        mem = tb(case.ints(r, 0, n), LENS)
        sb = {"original_shapes": shapes(LENS), "params_tb": mem}
        if r == SELF:
            case.given(sb)
        local = comp.compress(sb, residual=residual)
        if r == SELF:
            case.after("compress", dict(sb, **{"<returned>": local}))
        comp.sync(sb)
        if r == SELF:
            case.after("sync", sb)
            agg_tb = comp.uncompress(sb, WEIGHTS)
            case.after("uncompress", dict(sb, **{"<returned>": agg_tb}))
            case.state(memory=mem.buffer, aggregate=agg_tb.buffer)
            if local is not None:
                case.state(local=local.buffer)


def ef_sign(case, residual=False):
    from chocosgd_amd.ef_sign import EFSignCompressor
    n = sum(LENS)
    for r, agg in case.ranks():
        comp = EFSignCompressor(rank=r, world_size=3, aggregator=agg, comm_op="sign", comm_device="gpu",
                                use_ipc=False)
        grads = tb(case.ints(r, 0, n), LENS)
        sb = comp.compress(grads, residual=residual)
        if r == SELF:
            case.after("compress", sb)
        comp.sync(sb)
        if r == SELF:
            case.after("sync", sb)
            out = comp.decompress(sb)
            case.after("decompress", dict(sb, **{"<returned>": out}))
            case.state(grads=grads.buffer, synced=out.buffer)


def dgc(case, op):
    from chocosgd_amd.dgc import DGCCodec
    n = sum(LENS)
    for r, agg in case.ranks():
        comm_op = OPS[op]["comm_op"]
        comp = DGCCodec(agg, comm_op, "gpu", 3, quantize_level=4, is_biased=False, strict_reference=False)
        grads = list(tb(case.ints(r, 0, n), LENS))
        mem = tb(case.ints(r, 1, n), LENS)
        values, indices, n_bits = comp.compress(grads, mem, 0.9)
        synced, size = comp.sync(values, indices)
        if r == SELF:
            params = case.ints(r, 2, n)
            new = comp.recover_info(params, synced, size, 0.125)
            case.after("compress", {"values": values, "indices": indices, "n_bits": n_bits,
                                    "selected_shapes": comp.selected_shapes, "last_indices": comp.last_indices})
            case.after("sync", {"synced_message": synced, "message_size": size})
            case.after("recover_info", {"<returned>": new})
            case.state(memory=mem.buffer, params=params, new_params=new)


def _cases():
    cases = {}
    for op in OPS:
        for gossip in (False, True):
            cases[f"choco-{op}" + ("-gossip" if gossip else "")] = (choco, dict(op=op, gossip=gossip), Loop)
        cases[f"dcd-{op}"] = (dcd, dict(op=op), Loop)
        cases[f"ecd-{op}"] = (ecd, dict(op=op), Loop)
        for residual in (False, True):
            cases[f"deepsqueeze-{op}" + ("-residual" if residual else "")] = (
                deep_squeeze, dict(op=op, residual=residual), Loop)
    cases["choco-qsgd4-chunks2"] = (choco, dict(op="qsgd4", chunks=2), Loop)
    cases["choco-sign-chunks2-out"] = (choco, dict(op="sign", chunks=2), LoopOut)
    cases["choco-sign-chunks2-reassembled"] = (choco, dict(op="sign", chunks=2), Loop)
    for op in ("qsgd4", "sign"):
        cases[f"choco-{op}-deferred"] = (choco, dict(op=op, gossip=True, steps=2), Loop)
    for residual in (False, True):
        cases["efsign" + ("-residual" if residual else "")] = (ef_sign, dict(residual=residual), Loop)
    cases["dgc-top_k"] = (dgc, dict(op="top_k"), Loop)
    cases["dgc-qsgd4"] = (dgc, dict(op="qsgd4"), Loop)
    return cases


CASES = _cases()
NAMES = sorted(CASES)


def run_case(name, monkeypatch, names):
    """The record of one case with the functions `names` of codec.py traced."""
    fn, kw, agg_cls = CASES[name]
    case = Case(monkeypatch, names, NAMES.index(name), agg_cls)
    fn(case, **kw)
    return case.result()
