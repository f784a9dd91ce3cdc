"""Tensor-level entry points of the MI355X CHOCO codec.

Thin, allocation-light wrappers over the C ABI (include/choco_codec.h): they
validate that every tensor is a contiguous ROCm device tensor, allocate the
outputs with torch, pass raw pointers + the current HIP stream, and raise
RuntimeError on any library error.  CPU tensors are rejected -- there is no CPU
fallback anywhere in the product path.
"""
import ctypes
import math
import threading
import weakref

import torch

from . import _lib

_ws_lock = threading.Lock()
_ws_cache = {}


def _require(t, dtype=None, name="tensor"):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(
            f"chocosgd_amd runs on ROCm device tensors only; {name} is on {t.device}")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    return t


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _new_workspace(dev, nbytes):
    """A zero-filled workspace; the library forgets any warm-start record it kept for
    that address range (a freed workspace's address can come back)."""
    buf = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    lib().choco_topk_workspace_reset(_ptr(buf), buf.numel())
    return buf


def workspace(dev, kind, nbytes):
    """Per (device, stream, kind) scratch buffer; zero-filled on allocation.

    The sign/qsgd accumulators rely on starting zeroed; every kernel that uses
    them leaves them zeroed again (self-cleaning), so the buffer is reused as is.
    A top-k workspace also carries the warm-start window from one call to the next
    (include/choco_codec.h).
    """
    nbytes = max(int(nbytes), 256)
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, kind)
    with _ws_lock:
        buf = _ws_cache.get(key)
        if buf is None or buf.numel() < nbytes:
            if buf is not None:
                torch.cuda.current_stream(dev).synchronize()
                _status.pop(buf.data_ptr(), None)
            buf = _new_workspace(dev, nbytes)
            _ws_cache[key] = buf
        return buf


class TopkStatus:
    """Check of a top-k workspace's sticky status word (include/choco_codec.h,
    CHOCO_TOPK_STATUS_OFFSET) through its pinned host mirror: the device raises the bits
    there with a system-scope store, so `check()` -- called before every top-k call --
    reads host memory only (no copy on the stream, no synchronisation) and raises
    RuntimeError as soon as a call whose bounded fallback wait gave up has run on the GPU;
    that call's output (and whatever was computed from it: the model state of a CHOCO step
    that applied it) is invalid.  `check(wait=True)` first waits for the stream (teardown,
    checkpoints).  Holds the workspace's address only, never the tensor: a dropped
    workspace or SegmentPlan frees its device memory."""

    def __init__(self, ws):
        self.ptr = ws.data_ptr()
        self.device = ws.device
        # the stream the workspace belongs to (workspaces are per (device, stream): it is the
        # current stream when the workspace is taken, codec.workspace / SegmentPlan.workspace)
        self.stream = torch.cuda.current_stream(ws.device)

    def check(self, wait=False):
        if wait:
            self.stream.synchronize()
        bad = int(lib().choco_topk_host_status(ctypes.c_void_p(self.ptr), 1, _stream(self.device)))
        if bad < 0:
            raise RuntimeError(f"choco_topk_host_status failed: {_lib.last_error()}")
        if bad:
            raise RuntimeError(f"top-k: status word {bad:#x}: a bounded wait of the exact fallback gave up, so the "
                               "output of an earlier call on this workspace is invalid (and every state it was "
                               "applied to)")


_status = {}


def topk_status(ws):
    """The TopkStatus of a workspace tensor (one per workspace address)."""
    st = _status.get(ws.data_ptr())
    if st is None:
        st = _status[ws.data_ptr()] = TopkStatus(ws)
    return st


def check_topk_status(wait=True):
    """Check every top-k workspace's status word now (raises RuntimeError)."""
    for st in list(_status.values()):
        st.check(wait=wait)


def topk_fallback_count(dev=None, plan=None):
    """Diagnostic: calls on this stream's flat top-k workspace that took the exact fallback,
    or (plan=...) segments of that plan whose warm window missed (include/choco_codec.h
    CHOCO_TOPK_FALLBACKS_OFFSET).  Synchronises the stream."""
    return topk_workspace_word(_lib.TOPK_FALLBACKS_OFFSET, dev=dev, plan=plan)


def workspace_bytes():
    """Device bytes held by the cached scratch buffers (top-k: ~9 bytes per element of
    the largest flat input, sized for 288 GB HBM rather than packed)."""
    with _ws_lock:
        return sum(b.numel() for b in _ws_cache.values())


def drop_workspace(dev, kind):
    """Forget this stream's cached `kind` workspace (after a call sequence failed part-way:
    e.g. the sign / QSGD accumulators of an interrupted chunked pack are no longer zero);
    the next call allocates a fresh zero-filled one."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, kind)
    with _ws_lock:
        buf = _ws_cache.pop(key, None)
    if buf is not None:
        torch.cuda.current_stream(dev).synchronize()
        _status.pop(buf.data_ptr(), None)
        lib().choco_topk_workspace_reset(_ptr(buf), buf.numel())


def release_workspaces(dev=None):
    """Drop the cached scratch buffers (all devices, or `dev`) after synchronising the
    streams that used them; the next call on that stream allocates a fresh, zeroed one.
    SegmentPlan workspaces belong to their plan and go with it."""
    with _ws_lock:
        for key in list(_ws_cache):
            if dev is not None and key[0] != torch.device(dev).index:
                continue
            torch.cuda.synchronize(key[0])
            buf = _ws_cache.pop(key)
            _status.pop(buf.data_ptr(), None)
            lib().choco_topk_workspace_reset(_ptr(buf), buf.numel())


def lib():
    return _lib.load()


def _gossip(gossip, x, xhat):
    """`gossip=(memory, gamma)`: the fused consensus step x += gamma * (memory - xhat)
    (optim/utils.py:67-72) in the compressor's first pass; x is written in place and
    the codec compresses d = x_new - xhat (include/choco_codec.h)."""
    if gossip is None:
        return None
    memory, gamma = gossip
    _require(memory, torch.float32, "memory")
    if xhat is None:
        raise RuntimeError("the fused gossip step needs xhat")
    if memory.numel() != x.numel():
        raise RuntimeError("memory and x must have the same number of elements")
    return memory, float(gamma)


def _sparse_outputs(x, xhat, k, out, what="k"):
    """x (and xhat) checked, and the (values f32[k], indices i32[k]) outputs: the caller's
    `out` buffers, or fresh ones."""
    _require(x, torch.float32, "x")
    if xhat is not None:
        _require(xhat, torch.float32, "xhat")
        if xhat.numel() != x.numel():
            raise RuntimeError("x and xhat must have the same number of elements")
    if out is None:
        return (torch.empty(k, dtype=torch.float32, device=x.device),
                torch.empty(k, dtype=torch.int32, device=x.device))
    vals, idx = out
    _require(vals, torch.float32, "out values")
    _require(idx, torch.int32, "out indices")
    if vals.numel() != k or idx.numel() != k:
        raise RuntimeError(f"out buffers must hold exactly {what} elements")
    return vals, idx


# ----------------------------------------------------------------------------- top-k
def topk_k(n, ratio):
    """k = max(1, int(n * (1 - ratio))) (sparsification.py:22,45)."""
    return int(lib().choco_topk_k(int(n), float(ratio)))


def topk(x, k, xhat=None, out=None, gossip=None, fold=None):
    """Exact top-k by |x - xhat| (signed values, int32 indices, ascending index).

    `out=(values f32[k], indices i32[k])` writes into caller buffers (e.g. two views
    of one wire message) instead of allocating; `gossip=(memory, gamma)` fuses the
    consensus step (x is updated in place first).  `fold=(hat_self, memory, weight)`
    (either may be None) applies the self message's uncompress while the message is
    emitted: hat_self[idx] += v, memory[idx] += weight * v.  Folding memory is only
    bit-identical to the reference when the self rank is the first message applied to
    memory (include/choco_codec.h, choco_topk_compress_accumulate).  With `gossip`,
    hat_self must be xhat and memory the gossip memory (or None)."""
    vals, idx = _sparse_outputs(x, xhat, k, out)
    n = x.numel()
    dev = x.device
    L = lib()
    ws = workspace(dev, "topk", L.choco_topk_workspace_size(n))
    st = topk_status(ws)
    st.check()
    g = _gossip(gossip, x, xhat)
    if fold is not None:
        fhat, fmem, fw = fold
        for t, nm in ((fhat, "hat_self"), (fmem, "memory")):
            if t is not None:
                _require(t, torch.float32, nm)
                if t.numel() != n:
                    raise RuntimeError(f"{nm} and x must have the same number of elements")
        if fhat is None and fmem is None:
            raise RuntimeError("fold: hat_self and memory are both None")
        if g is not None:
            if fhat is None or fhat.data_ptr() != xhat.data_ptr():
                raise RuntimeError("with gossip, the fold's hat_self must be xhat")
            if fmem is not None and fmem.data_ptr() != g[0].data_ptr():
                raise RuntimeError("with gossip, the folded memory must be the gossip memory")
            _lib.check(L.choco_gossip_topk_compress_accumulate(
                _ptr(x), _ptr(g[0]), _ptr(xhat), g[1], n, int(k), _ptr(vals), _ptr(idx), int(fmem is not None),
                float(fw), _ptr(ws), ws.numel(), _stream(dev)), "choco_gossip_topk_compress_accumulate")
        else:
            _lib.check(L.choco_topk_compress_accumulate(
                _ptr(x), _ptr(xhat), n, int(k), _ptr(vals), _ptr(idx), _ptr(fhat), _ptr(fmem), float(fw),
                _ptr(ws), ws.numel(), _stream(dev)), "choco_topk_compress_accumulate")
    elif g is not None:
        _lib.check(L.choco_gossip_topk_compress(_ptr(x), _ptr(g[0]), _ptr(xhat), g[1], n, int(k), _ptr(vals),
                                                _ptr(idx), _ptr(ws), ws.numel(), _stream(dev)),
                   "choco_gossip_topk_compress")
    else:
        _lib.check(L.choco_topk_compress(_ptr(x), _ptr(xhat), n, int(k), _ptr(vals), _ptr(idx), _ptr(ws),
                                         ws.numel(), _stream(dev)), "choco_topk_compress")
    return vals, idx


class SegmentPlan:
    """Host + device copies of the per-segment top-k plan (include/choco_codec.h):
    rows {off, len, k, out_off, first tile, tiles, ..} + the tile -> segment map."""

    def __init__(self, seg_lens, ratio, device):
        L = lib()
        self.seg_lens = [int(s) for s in seg_lens]
        self.nseg = len(self.seg_lens)
        offs = [0]
        for s in self.seg_lens:
            offs.append(offs[-1] + s)
        self.seg_off = offs
        self.n = offs[-1]
        p_off, self._off_keep = _lib.i64_array(offs)
        plen = L.choco_topk_segmented_plan_len(p_off, self.nseg)
        if plen < 0:
            raise RuntimeError(f"choco_topk_segmented_plan_len failed: {_lib.last_error()}")
        self._plan_host = (ctypes.c_int64 * int(plen))()
        self.plan_host = ctypes.cast(self._plan_host, ctypes.POINTER(ctypes.c_int64))
        total = L.choco_topk_segmented_plan(p_off, self.nseg, float(ratio), self.plan_host)
        if total < 0:
            raise RuntimeError(f"choco_topk_segmented_plan failed: {_lib.last_error()}")
        self.k_total = int(total)
        self.k_per_seg = [int(self._plan_host[8 * s + 2]) for s in range(self.nseg)]
        self.ntile = int(self._plan_host[6])
        self.plan_dev = torch.tensor(list(self._plan_host), dtype=torch.int64, device=device)
        self.ws_bytes = int(L.choco_topk_segmented_workspace_size(self.plan_host, self.nseg))
        self._base = None
        self._ws = {}

    def workspace(self, dev):
        """This plan's own zero-filled workspace per stream: the batched select keeps
        per-segment histograms there that every call leaves zeroed for the NEXT call of
        the same plan (include/choco_codec.h), so no other call may share it."""
        key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
        with _ws_lock:
            buf = self._ws.get(key)
            if buf is None:
                buf = self._ws[key] = _new_workspace(dev, max(self.ws_bytes, 256))
            return buf

    def __del__(self):
        # The plan's workspaces go with it, and so does the codec's host-side state keyed by
        # their addresses (warm windows, the pinned miss flag): a later workspace at the
        # same address must not inherit it.  The device may still write the miss flag, so
        # the devices are synchronised before it is freed.
        try:
            bufs = list(self._ws.values())
            self._ws.clear()
            if not bufs:
                return
            for d in {b.device.index for b in bufs}:
                torch.cuda.synchronize(d)
            L = lib()
            for buf in bufs:
                _status.pop(buf.data_ptr(), None)
                L.choco_topk_workspace_reset(_ptr(buf), buf.numel())
        except Exception:  # interpreter shutdown: the library or torch may be gone
            pass

    def drop_workspace(self, dev):
        """Forget this plan's workspace on the current stream of `dev` (after a failed
        call: its histograms may not be zeroed any more); the next call starts cold on
        a fresh zero-filled one."""
        key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
        with _ws_lock:
            buf = self._ws.pop(key, None)
        if buf is not None:
            _status.pop(buf.data_ptr(), None)
            lib().choco_topk_workspace_reset(_ptr(buf), buf.numel())

    def selected_base(self):
        """int32[K]: the segment start of every output slot (global -> local index)."""
        if self._base is None:
            offs = torch.tensor(self.seg_off[:-1], dtype=torch.int32, device=self.plan_dev.device)
            ks = torch.tensor(self.k_per_seg, dtype=torch.int64, device=self.plan_dev.device)
            self._base = torch.repeat_interleave(offs, ks)
        return self._base


def _seg_outputs(x, xhat, plan, out):
    _require(x, torch.float32, "x")
    if x.numel() != plan.n:
        raise RuntimeError(f"x holds {x.numel()} elements, the segment plan {plan.n}")
    return _sparse_outputs(x, xhat, plan.k_total, out, what="the plan's K")


def topk_segmented(x, plan, xhat=None, out=None, gossip=None):
    """Per-segment top-k (k_s of the plan), GLOBAL int32 indices; `out=(values, indices)`
    writes into caller buffers (e.g. the two halves of a wire message);
    `gossip=(memory, gamma)` fuses the consensus step."""
    vals, idx = _seg_outputs(x, xhat, plan, out)
    dev = x.device
    L = lib()
    ws = plan.workspace(dev)
    st = topk_status(ws)
    st.check()
    g = _gossip(gossip, x, xhat)
    try:
        if g is not None:
            _lib.check(L.choco_gossip_topk_compress_segmented(_ptr(x), _ptr(g[0]), _ptr(xhat), g[1],
                                                              _ptr(plan.plan_dev), plan.plan_host, plan.nseg,
                                                              _ptr(vals), _ptr(idx), _ptr(ws), ws.numel(),
                                                              _stream(dev)),
                       "choco_gossip_topk_compress_segmented")
        else:
            _lib.check(L.choco_topk_compress_segmented(_ptr(x), _ptr(xhat), _ptr(plan.plan_dev), plan.plan_host,
                                                       plan.nseg, _ptr(vals), _ptr(idx), _ptr(ws), ws.numel(),
                                                       _stream(dev)), "choco_topk_compress_segmented")
    except RuntimeError:
        # a call that failed part-way may leave the plan's histograms non-zero
        torch.cuda.synchronize(dev)
        plan.drop_workspace(dev)
        raise
    return vals, idx


# ----------------------------------------------------------------------------- random-k
def randk(x, k, seed, is_biased=True, xhat=None, offset=0, out=None):
    """Uniform random k-subset (include/choco_codec.h: the device sampler of (seed, offset)),
    values x[i] (- xhat[i]) (* n / k unbiased), int32 indices in ascending order;
    `out=(values f32[k], indices i32[k])` writes into caller buffers."""
    vals, idx = _sparse_outputs(x, xhat, k, out)
    n = x.numel()
    dev = x.device
    L = lib()
    ws = workspace(dev, "randk", L.choco_randk_workspace_size(n))
    _lib.check(L.choco_randk_compress(_ptr(x), _ptr(xhat), n, int(k), int(seed) & (2**64 - 1),
                                      int(offset) & (2**64 - 1), 1 if is_biased else 0, _ptr(vals), _ptr(idx),
                                      _ptr(ws), ws.numel(), _stream(dev)), "choco_randk_compress")
    return vals, idx


def randk_segmented(x, plan, seed, is_biased=True, xhat=None, out=None, gossip=None, offset=0):
    """Per-segment random-k over a SegmentPlan (k_s as top-k's), one batched call:
    segment s drawn with key derive(key(seed, offset), s); GLOBAL indices."""
    vals, idx = _seg_outputs(x, xhat, plan, out)
    dev = x.device
    L = lib()
    ws = plan.workspace(dev)
    g = _gossip(gossip, x, xhat)
    sd, off = int(seed) & (2**64 - 1), int(offset) & (2**64 - 1)
    if g is not None:
        _lib.check(L.choco_gossip_randk_compress_segmented(_ptr(x), _ptr(g[0]), _ptr(xhat), g[1],
                                                           _ptr(plan.plan_dev), plan.plan_host, plan.nseg, sd, off,
                                                           1 if is_biased else 0, _ptr(vals), _ptr(idx), _ptr(ws),
                                                           ws.numel(), _stream(dev)),
                   "choco_gossip_randk_compress_segmented")
    else:
        _lib.check(L.choco_randk_compress_segmented(_ptr(x), _ptr(xhat), _ptr(plan.plan_dev), plan.plan_host,
                                                    plan.nseg, sd, off, 1 if is_biased else 0, _ptr(vals), _ptr(idx),
                                                    _ptr(ws), ws.numel(), _stream(dev)),
                   "choco_randk_compress_segmented")
    return vals, idx


def gather(x, idx, scale=1.0, xhat=None):
    _require(x, torch.float32, "x")
    _require(idx, torch.int64, "idx")
    out = torch.empty(idx.numel(), dtype=torch.float32, device=x.device)
    _lib.check(lib().choco_gather(_ptr(x), _ptr(xhat), _ptr(idx), idx.numel(), float(scale), _ptr(out),
                                  _stream(x.device)), "choco_gather")
    return out


class IndexGuard:
    """Lazy check of the out-of-range index count that the sparse accumulate
    keeps in a device word (include/choco_codec.h): `arm()` queues a
    non-blocking copy of the word to pinned host memory behind the launches;
    `check()` raises RuntimeError -- the reference's index_put raises
    IndexError -- once that copy has landed with a count above what was already
    reported.  The count is cumulative (never reset on the device), so no error is
    lost between copies.  No host synchronisation on the hot path; callers check
    AFTER their own step's work is queued (a bad index of an earlier step must not
    stop this step's valid messages from being applied), and `check(wait=True)`
    copies and waits (teardown, checkpoints)."""

    def __init__(self, device):
        self.device = device
        self.word = torch.zeros(1, dtype=torch.int32, device=device)
        self.host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.event = None
        self.reported = 0

    def arm(self):
        self.host.copy_(self.word, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(self.device))

    def check(self, wait=False):
        if wait and self.event is None:
            self.arm()
        if self.event is None:
            return
        if wait:
            self.event.synchronize()
        elif not self.event.query():
            return
        self.event = None
        bad = int(self.host.item()) & 0xFFFFFFFF
        if bad > self.reported:
            new, self.reported = bad - self.reported, bad
            raise RuntimeError(f"sparse accumulate: {new} received indices out of range or not ascending (corrupt "
                               "message or a peer with a different parameter layout); a corrupt message may already "
                               "have been applied")

    def check_then_arm(self):
        """End of a receiver step: report an EARLIER step's bad indices (this step's
        messages are already applied), then queue this step's copy."""
        try:
            self.check()
        finally:
            self.arm()


MAX_SPARSE_MSGS = 8  # messages per choco_sparse_accumulate_multi call


def sparse_accumulate_multi(messages, weights, memory, self_slot=-1, xhat_self=None, guard=None):
    """Every message of a receive step in ONE call (include/choco_codec.h
    choco_sparse_accumulate_multi): for m in order, x_hat[idx_m] += v_m (m == self_slot,
    xhat_self given) and memory[idx_m] += weights[m] * v_m -- bit-identical to one
    sparse_accumulate per message in that order (the per-message kernels run it).  messages: [(values f32, indices i32)];
    any count (chunks of MAX_SPARSE_MSGS, applied in order)."""
    _require(memory, torch.float32, "memory")
    if len(messages) != len(weights):
        raise RuntimeError("one weight per message")
    for v, i in messages:
        _require(v, torch.float32, "values")
        _require(i, torch.int32, "indices")
        if v.numel() != i.numel():
            raise RuntimeError("values and indices must have the same length")
    if xhat_self is not None:
        _require(xhat_self, torch.float32, "xhat_self")
        if xhat_self.numel() != memory.numel():
            raise RuntimeError("xhat_self and memory must have the same length")
    n = memory.numel()
    L = lib()
    dev = memory.device
    for c0 in range(0, len(messages), MAX_SPARSE_MSGS):
        part = messages[c0:c0 + MAX_SPARSE_MSGS]
        m = len(part)
        slot = self_slot - c0 if (xhat_self is not None and c0 <= self_slot < c0 + m) else -1
        nws = L.choco_sparse_accumulate_multi_workspace_size(n, m)
        ws = workspace(dev, "accm", nws) if nws else None
        vp, keep1 = _lib.ptr_array([v.data_ptr() for v, _ in part])
        ip, keep2 = _lib.ptr_array([i.data_ptr() for _, i in part])
        kp, keep3 = _lib.i64_array([v.numel() for v, _ in part])
        wp, keep4 = _lib.f32_array([float(w) for w in weights[c0:c0 + m]])
        _lib.check(L.choco_sparse_accumulate_multi(vp, ip, kp, wp, m, slot, _ptr(xhat_self if slot >= 0 else None),
                                                   _ptr(memory), n, _ptr(ws), ws.numel() if ws is not None else 0,
                                                   _ptr(guard.word) if guard is not None else ctypes.c_void_p(0),
                                                   _stream(dev)),
                   "choco_sparse_accumulate_multi")


def sparse_accumulate(values, indices, memory, weight, xhat_self=None, guard=None):
    """x_hat[idx] += v (xhat_self given); memory[idx] += weight * v.  Indices
    outside memory are skipped and counted into `guard` (an IndexGuard)."""
    _require(values, torch.float32, "values")
    _require(indices, torch.int32, "indices")
    _require(memory, torch.float32, "memory")
    if indices.numel() != values.numel():
        raise RuntimeError("values and indices must have the same length")
    if xhat_self is not None:
        _require(xhat_self, torch.float32, "xhat_self")
        if xhat_self.numel() != memory.numel():
            raise RuntimeError("xhat_self and memory must have the same length")
    _lib.check(lib().choco_sparse_accumulate(_ptr(values), _ptr(indices), values.numel(), _ptr(xhat_self),
                                             _ptr(memory), memory.numel(), float(weight),
                                             _ptr(guard.word) if guard is not None else ctypes.c_void_p(0),
                                             _stream(memory.device)),
               "choco_sparse_accumulate")


def sparse_extrapolate(values, indices, target, a, b, guard=None):
    """target[idx] = fmaf(b, v, target[idx] * a): ECD's replica update (ecd_psgd.py:299-303)."""
    _require(values, torch.float32, "values")
    _require(indices, torch.int32, "indices")
    _require(target, torch.float32, "target")
    if indices.numel() != values.numel():
        raise RuntimeError("values and indices must have the same length")
    _lib.check(lib().choco_sparse_extrapolate(_ptr(values), _ptr(indices), values.numel(), _ptr(target),
                                              target.numel(), float(a), float(b),
                                              _ptr(guard.word) if guard is not None else ctypes.c_void_p(0),
                                              _stream(target.device)), "choco_sparse_extrapolate")


# ----------------------------------------------------------------------------- sign
def sign_words(n):
    return int(lib().choco_sign_words(int(n)))


def _out_views(out, packed_n, packed_dtype, nseg, dev):
    """Caller-provided (packed, norms) buffers -- e.g. views into one wire message, so the
    kernels write the message in place instead of a torch.cat copying it afterwards."""
    packed, norms = out
    _require(packed, packed_dtype, "out packed")
    if packed.numel() != packed_n or packed.device != dev:
        raise RuntimeError(f"out packed must hold {packed_n} elements on {dev}")
    if norms is not None:
        _require(norms, torch.float32, "out norms")
        if norms.numel() != nseg or norms.device != dev:
            raise RuntimeError(f"out norms must hold {nseg} floats on {dev}")
    return packed, norms


def wire_header_words(nseg):
    """int32 words of a wire message's fp32 norms header (16-byte aligned)."""
    return (int(nseg) + 3) // 4 * 4


def sign_wire(n, nseg, dev):
    """One sign wire message [fp32 norms (16-B padded) | int32 words[N']] and the
    (packed, norms) views sign_compress(out=...) fills in place (header pad zeroed)."""
    hw = wire_header_words(nseg)
    msg = torch.empty(hw + sign_words(n), dtype=torch.int32, device=dev)
    msg[:hw].zero_()
    return msg, (msg[hw:], msg[:hw].view(torch.float32)[:nseg])


def sign_split(message, nseg):
    """A received sign wire message taken apart: (int32 words, fp32 norms[nseg]), views of it."""
    hw = wire_header_words(nseg)
    return message[hw:], message[:hw].view(torch.float32)[:nseg].contiguous()


def sparse_wire(k, dev):
    """One sparse wire message [fp32 values[k] | int32 global indices[k]] and the (values,
    indices) views topk_segmented / randk_segmented(out=...) fill in place."""
    msg = torch.empty(2 * k, dtype=torch.int32, device=dev)
    return msg, sparse_split(msg)


def sparse_split(message, size=None):
    """A sparse wire message taken apart: (fp32 values, int32 indices), views of it.  `size`:
    the length every message of the exchange has (the sender's own), default this one's."""
    k = (message.numel() if size is None else int(size)) // 2
    return message[:k].view(torch.float32), message[k:]


def sign_compress(x, xhat=None, seg_off=None, nseg=1, want_norms=True, gossip=None, out=None):
    """Pack sign bits in the (32, N') layout; optionally per-segment L1 norms (fp64-accumulated).
    `gossip=(memory, gamma)` fuses the consensus step; `out=(packed int32[N'], norms f32[nseg])`
    writes into caller buffers."""
    _require(x, torch.float32, "x")
    if xhat is not None:
        _require(xhat, torch.float32, "xhat")
    if seg_off is not None:
        _require(seg_off, torch.int64, "seg_off")
    n = x.numel()
    dev = x.device
    L = lib()
    if out is not None:
        packed, norms = _out_views(out, sign_words(n), torch.int32, nseg, dev)
    else:
        packed = torch.empty(sign_words(n), dtype=torch.int32, device=dev)
        norms = torch.empty(nseg, dtype=torch.float32, device=dev) if want_norms else None
    ws = workspace(dev, "acc", L.choco_sign_workspace_size(nseg))
    g = _gossip(gossip, x, xhat)
    if g is not None:
        _lib.check(L.choco_gossip_sign_compress(_ptr(x), _ptr(g[0]), _ptr(xhat), g[1], n, _ptr(seg_off), int(nseg),
                                                _ptr(packed), _ptr(norms), _ptr(ws), ws.numel(), _stream(dev)),
                   "choco_gossip_sign_compress")
        return packed, norms
    _lib.check(L.choco_sign_compress(_ptr(x), _ptr(xhat), n, _ptr(seg_off), int(nseg), _ptr(packed), _ptr(norms),
                                     _ptr(ws), ws.numel(), _stream(dev)), "choco_sign_compress")
    return packed, norms


SIGN_RANGE_ALIGN = 1024  # words per pack workgroup (sign.hip kSignCols)


def sign_chunks(n, chunks):
    """`chunks` word ranges [(w0, w1)] covering [0, N'), starts aligned to 1024 words."""
    words = sign_words(n)
    per = -(-words // max(1, int(chunks)))
    per = -(-per // SIGN_RANGE_ALIGN) * SIGN_RANGE_ALIGN
    return [(w, min(w + per, words)) for w in range(0, words, per)]


def sign_compress_range(x, w0, w1, finish, xhat=None, seg_off=None, nseg=1, gossip=None, out=None):
    """Pack the words [w0, w1) of sign_compress's layout into out=(packed int32[N'], norms
    f32[nseg] or None); the norms are written by the `finish` call, which must be the last
    range of the message on this stream (include/choco_codec.h "Chunked sign pack")."""
    _require(x, torch.float32, "x")
    if xhat is not None:
        _require(xhat, torch.float32, "xhat")
    if seg_off is not None:
        _require(seg_off, torch.int64, "seg_off")
    n = x.numel()
    dev = x.device
    L = lib()
    packed, norms = _out_views(out, sign_words(n), torch.int32, nseg, dev)
    ws = workspace(dev, "acc", L.choco_sign_workspace_size(nseg))
    g = _gossip(gossip, x, xhat)
    fin = 1 if finish else 0
    if g is not None:
        _lib.check(L.choco_gossip_sign_compress_range(_ptr(x), _ptr(g[0]), _ptr(xhat), g[1], n, _ptr(seg_off),
                                                      int(nseg), int(w0), int(w1), fin, _ptr(packed), _ptr(norms),
                                                      _ptr(ws), ws.numel(), _stream(dev)),
                   "choco_gossip_sign_compress_range")
    else:
        _lib.check(L.choco_sign_compress_range(_ptr(x), _ptr(xhat), n, _ptr(seg_off), int(nseg), int(w0), int(w1),
                                               fin, _ptr(packed), _ptr(norms), _ptr(ws), ws.numel(), _stream(dev)),
                   "choco_sign_compress_range")
    return packed, norms


def sign_unpack(packed, n):
    _require(packed, torch.int32, "packed")
    out = torch.empty(n, dtype=torch.float32, device=packed.device)
    _lib.check(lib().choco_sign_unpack(_ptr(packed), int(n), _ptr(out), _stream(packed.device)),
               "choco_sign_unpack")
    return out


MAX_FUSED_MSGS = 8  # messages one fused accumulate launch takes (sign.hip kMaxMsg, qsgd.hip kQMaxMsg)


def _msg_tables(messages, weights, self_slot, dtype, kind, size, unit, nseg):
    """Checks the [(packed, norms)] messages of a multi-message call (`size` `unit`s of `dtype`
    and nseg norms each, one weight per message) and returns the C tables of its launches:
    [(packed**, norms**, weights*, count, slot, keep-alive)] for consecutive chunks of
    <= MAX_FUSED_MSGS messages, in order, with the local slot re-based into its chunk (-1
    elsewhere).  memory is updated message by message, so chunked launches give the same fp32
    sequence as one launch."""
    if len(messages) != len(weights):
        raise RuntimeError("one weight per message")
    for p, nm in messages:
        _require(p, dtype, "packed")
        _require(nm, torch.float32, "norms")
        if p.numel() != size or nm.numel() != nseg:
            raise RuntimeError(f"{kind} message must hold {size} {unit} and {nseg} norms, got {p.numel()} / "
                               f"{nm.numel()}")
    self_slot = int(self_slot)
    calls = []
    for c0 in range(0, len(messages), MAX_FUSED_MSGS):
        part = messages[c0:c0 + MAX_FUSED_MSGS]
        pp, keep1 = _lib.ptr_array([p.data_ptr() for p, _ in part])
        nn, keep2 = _lib.ptr_array([nm.data_ptr() for _, nm in part])
        ww, keep3 = _lib.f32_array([float(w) for w in weights[c0:c0 + len(part)]])
        slot = self_slot - c0 if c0 <= self_slot < c0 + len(part) else -1
        calls.append((pp, nn, ww, len(part), slot, (keep1, keep2, keep3)))
    return calls


def _check_layout(memory, xhat_self, n, seg_off, nseg):
    if memory.numel() != n:
        raise RuntimeError(f"memory holds {memory.numel()} elements, the messages describe {n}")
    if xhat_self is not None:
        _require(xhat_self, torch.float32, "xhat_self")
        if xhat_self.numel() != n:
            raise RuntimeError("xhat_self and memory must have the same length")
    if nseg > 1:
        _require(seg_off, torch.int64, "seg_off")
        if seg_off.numel() != nseg + 1:
            raise RuntimeError("seg_off must hold nseg + 1 offsets")


def sign_accumulate(messages, weights, self_slot, n, memory, xhat_self=None, seg_off=None, nseg=1):
    """messages: list of (packed int32[N'], norms f32[nseg]) applied in order; any count
    (launched in fused chunks of MAX_FUSED_MSGS)."""
    _require(memory, torch.float32, "memory")
    _check_layout(memory, xhat_self, n, seg_off, nseg)
    for pp, nn, ww, m, slot, _keep in _msg_tables(messages, weights, self_slot, torch.int32, "sign", sign_words(n),
                                                  "words", nseg):
        _lib.check(lib().choco_sign_decompress_accumulate(pp, nn, ww, m, slot, int(n), _ptr(seg_off),
                                                          int(nseg), _ptr(xhat_self if slot >= 0 else None),
                                                          _ptr(memory), ctypes.c_void_p(0), 0,
                                                          _stream(memory.device)),
                   "choco_sign_decompress_accumulate")


def sign_recv_gossip_compress(messages, weights, self_slot, x, memory, xhat, gamma, seg_off=None, nseg=1,
                              out=None):
    """The deferred receive fused into the next step's pass (include/choco_codec.h
    choco_sign_recv_gossip_compress): the previous step's messages [(packed, norms)] into
    x_hat (self_slot) and memory in order, then x += gamma (memory - x_hat), then this step's
    message (packed signs of x - x_hat, L1 norms) -- returned, or written to
    `out=(packed, norms)`, which must not be one of `messages`' buffers.  More than 8
    messages: the leading chunks are applied by sign_accumulate first (same order)."""
    _require(x, torch.float32, "x")
    _require(xhat, torch.float32, "xhat")
    _require(memory, torch.float32, "memory")
    n = x.numel()
    _check_layout(memory, xhat, n, seg_off, nseg)
    if len(messages) != len(weights) or not messages:
        raise RuntimeError("one weight per message, at least one message")
    words = sign_words(n)
    head = max(0, len(messages) - MAX_FUSED_MSGS)  # leading messages: applied first, in order
    (pp, nn, ww, m, slot, _keep), = _msg_tables(messages[head:], weights[head:], self_slot - head, torch.int32, "sign",
                                                words, "words", nseg)
    dev = x.device
    if out is not None:
        packed, norms = _out_views(out, words, torch.int32, nseg, dev)
    else:
        packed = torch.empty(words, dtype=torch.int32, device=dev)
        norms = torch.empty(nseg, dtype=torch.float32, device=dev)
    if head > 0:
        sign_accumulate(messages[:head], weights[:head], self_slot, n, memory,
                        xhat_self=xhat if 0 <= self_slot < head else None, seg_off=seg_off, nseg=nseg)
    L = lib()
    # (its own workspace: the accumulator block plus bit planes of the messages and the output)
    ws = workspace(dev, "signrecv", L.choco_sign_recv_workspace_size(n, nseg, m))
    _lib.check(L.choco_sign_recv_gossip_compress(pp, nn, ww, m, slot, _ptr(x), _ptr(memory), _ptr(xhat),
                                                 float(gamma), n, _ptr(seg_off), int(nseg), _ptr(packed),
                                                 _ptr(norms), _ptr(ws), ws.numel(), _stream(dev)),
               "choco_sign_recv_gossip_compress")
    return packed, norms


def sign_axpy(messages, weights, n, target, seg_off=None, nseg=1, two_roundings=False):
    """target += w_m * decode(m) for each (packed, norms) message in order -- the receiver of
    the DCD / DeepSqueeze sign compressors; `two_roundings` selects torch's add_(w * u)
    over add_(u, alpha=w) (include/choco_codec.h)."""
    _require(target, torch.float32, "target")
    _check_layout(target, None, n, seg_off, nseg)
    for pp, nn, ww, m, _slot, _keep in _msg_tables(messages, weights, -1, torch.int32, "sign", sign_words(n), "words",
                                                   nseg):
        _lib.check(lib().choco_sign_decompress_axpy(pp, nn, ww, m, int(n), _ptr(seg_off), int(nseg),
                                                    1 if two_roundings else 0, _ptr(target),
                                                    _stream(target.device)), "choco_sign_decompress_axpy")


def sign_extrapolate(packed, norms, n, target, a, b, seg_off=None, nseg=1):
    """target_s = target_s * a + ((b * norm_s) / numel_s) * sign: ECD (ecd_psgd.py:448-454)."""
    _require(packed, torch.int32, "packed")
    _require(norms, torch.float32, "norms")
    _require(target, torch.float32, "target")
    _check_layout(target, None, n, seg_off, nseg)
    _lib.check(lib().choco_sign_decompress_extrapolate(_ptr(packed), _ptr(norms), int(n), _ptr(seg_off), int(nseg),
                                                       float(a), float(b), _ptr(target), _stream(target.device)),
               "choco_sign_decompress_extrapolate")


def sign_local_decode(x, norms, seg_off=None, nseg=1):
    """(norm_s * torch.sign(x)) / numel_s: DeepSqueeze's local copy of its sign message."""
    _require(x, torch.float32, "x")
    _require(norms, torch.float32, "norms")
    out = torch.empty_like(x)
    _lib.check(lib().choco_sign_local_decode(_ptr(x), x.numel(), _ptr(seg_off), int(nseg), _ptr(norms), _ptr(out),
                                             _stream(x.device)), "choco_sign_local_decode")
    return out


def sign_local_residual(x, norms, seg_off=None, nseg=1, local_out=None, resid_out=None):
    """The error feedback of a sign message in one pass: resid_out = x - u with u =
    sign_local_decode's value, and local_out = u when given (deep_squeeze.py:416-422 with :115;
    ef_sign_sgd.py:153 with :104-106).  resid_out may be x itself (in place; None: a new
    tensor); local_out may alias neither.  Returns resid_out."""
    _require(x, torch.float32, "x")
    _require(norms, torch.float32, "norms")
    if resid_out is None:
        resid_out = torch.empty_like(x)
    for name, t in (("local_out", local_out), ("resid_out", resid_out)):
        if t is not None:
            _require(t, torch.float32, name)
            if t.device != x.device or t.numel() != x.numel():
                raise RuntimeError(f"{name} must hold {x.numel()} elements on {x.device}")
    _lib.check(lib().choco_sign_local_residual(_ptr(x), x.numel(), _ptr(seg_off), int(nseg), _ptr(norms),
                                               _ptr(local_out), _ptr(resid_out), _stream(x.device)),
               "choco_sign_local_residual")
    return resid_out


# ----------------------------------------------------------------------------- QSGD
def qsgd_packed_bytes(n, q):
    return int(lib().choco_qsgd_packed_bytes(int(n), int(q)))


def qsgd_wire(n, q, nseg, dev):
    """One QSGD wire message [fp32 norms (16-B padded) | level plane | sign plane] (uint8)
    and the (packed, norms) views qsgd_compress(out=...) fills in place (header pad zeroed)."""
    hb = 4 * wire_header_words(nseg)
    msg = torch.empty(hb + qsgd_packed_bytes(n, q), dtype=torch.uint8, device=dev)
    msg[:hb].zero_()
    return msg, (msg[hb:], msg[:hb].view(torch.float32)[:nseg])


def qsgd_split(message, nseg):
    """A received QSGD wire message taken apart: (uint8 planes, fp32 norms[nseg]), views of it.
    The header of a chunked message (qsgd_chunked_wire), sent alone, gives its norms."""
    hb = 4 * wire_header_words(nseg)
    return message[hb:], message[:hb].view(torch.float32)[:nseg].contiguous()


def qsgd_compress(x, q, is_biased=False, xhat=None, seg_off=None, nseg=1, norm_in=None, u_in=None,
                  seed=0, offset=0, want_dense=False, gossip=None, out=None):
    """QSGD with s = 2^q - 1.  Returns (packed uint8, norms f32[nseg], dense f32[n] or None).
    `gossip=(memory, gamma)` fuses the consensus step (device norms and uniforms only);
    `out=(packed uint8[qsgd_packed_bytes], norms f32[nseg])` writes into caller buffers."""
    _require(x, torch.float32, "x")
    if xhat is not None:
        _require(xhat, torch.float32, "xhat")
    if seg_off is not None:
        _require(seg_off, torch.int64, "seg_off")
    if norm_in is not None:
        _require(norm_in, torch.float32, "norm_in")
    if u_in is not None:
        _require(u_in, torch.float32, "u_in")
        if u_in.numel() != x.numel():
            raise RuntimeError("u_in must have one uniform per element")
    n = x.numel()
    dev = x.device
    L = lib()
    if out is not None:
        packed, norms = _out_views(out, qsgd_packed_bytes(n, q), torch.uint8, nseg, dev)
        if norms is None:
            raise RuntimeError("out norms is required")
    else:
        packed = torch.empty(qsgd_packed_bytes(n, q), dtype=torch.uint8, device=dev)
        norms = torch.empty(nseg, dtype=torch.float32, device=dev)
    dense = torch.empty(n, dtype=torch.float32, device=dev) if want_dense else None
    ws = workspace(dev, "acc", L.choco_qsgd_workspace_size(nseg))
    g = _gossip(gossip, x, xhat)
    if g is not None:
        if norm_in is not None or u_in is not None:
            raise RuntimeError("the fused gossip step takes the device norms and uniforms")
        _lib.check(L.choco_gossip_qsgd_compress(_ptr(x), _ptr(g[0]), _ptr(xhat), g[1], n, _ptr(seg_off), int(nseg),
                                                int(q), 1 if is_biased else 0, int(seed) & (2**64 - 1),
                                                int(offset) & (2**64 - 1), _ptr(packed), _ptr(norms), _ptr(dense),
                                                _ptr(ws), ws.numel(), _stream(dev)), "choco_gossip_qsgd_compress")
        return packed, norms, dense
    _lib.check(L.choco_qsgd_compress(_ptr(x), _ptr(xhat), n, _ptr(seg_off), int(nseg), int(q),
                                     1 if is_biased else 0, _ptr(norm_in), _ptr(u_in), int(seed) & (2**64 - 1),
                                     int(offset) & (2**64 - 1), _ptr(packed), _ptr(norms), _ptr(dense), _ptr(ws),
                                     ws.numel(), _stream(dev)), "choco_qsgd_compress")
    return packed, norms, dense


def qsgd_decode(packed, norms, n, q, is_biased=False, seg_off=None, nseg=1):
    _require(packed, torch.uint8, "packed")
    _require(norms, torch.float32, "norms")
    out = torch.empty(n, dtype=torch.float32, device=packed.device)
    _lib.check(lib().choco_qsgd_decode(_ptr(packed), _ptr(norms), int(n), _ptr(seg_off), int(nseg), int(q),
                                       1 if is_biased else 0, _ptr(out), _stream(packed.device)),
               "choco_qsgd_decode")
    return out


def qsgd_accumulate(messages, weights, self_slot, n, q, memory, xhat_self=None, is_biased=False, seg_off=None,
                    nseg=1):
    """messages: list of (packed uint8, norms f32[nseg]) applied in order; any count
    (launched in fused chunks of MAX_FUSED_MSGS)."""
    _require(memory, torch.float32, "memory")
    _check_layout(memory, xhat_self, n, seg_off, nseg)
    for pp, nn, ww, m, slot, _keep in _msg_tables(messages, weights, self_slot, torch.uint8, "QSGD",
                                                  qsgd_packed_bytes(n, q), "bytes", nseg):
        _lib.check(lib().choco_qsgd_decompress_accumulate(pp, nn, ww, m, slot, int(n), _ptr(seg_off),
                                                          int(nseg), int(q), 1 if is_biased else 0,
                                                          _ptr(xhat_self if slot >= 0 else None), _ptr(memory),
                                                          _stream(memory.device)),
                   "choco_qsgd_decompress_accumulate")


# ---- chunked QSGD wire (include/choco_codec.h "Chunked QSGD wire")
QSGD_RANGE_ALIGN = 8192


def qsgd_chunks(n, chunks):
    """`chunks` element ranges [(e0, e1)] covering [0, n), starts aligned to 8192."""
    per = -(-int(n) // max(1, int(chunks)))
    per = -(-per // QSGD_RANGE_ALIGN) * QSGD_RANGE_ALIGN
    return [(e, min(e + per, n)) for e in range(0, n, per)]


def qsgd_chunked_wire(n, q, nseg, chunks, dev):
    """One chunked QSGD message [fp32 norms (16-B padded) | range 0 | range 1 | ...], each
    range a self-contained [level plane | sign plane]; returns (message, norms view,
    [(e0, e1, range view)])."""
    hb = 4 * wire_header_words(nseg)
    ranges = qsgd_chunks(n, chunks)
    offs = [hb]
    for e0, e1 in ranges:
        offs.append(offs[-1] + qsgd_packed_bytes(e1 - e0, q))
    msg = torch.empty(offs[-1], dtype=torch.uint8, device=dev)
    msg[:hb].zero_()
    parts = [(e0, e1, msg[offs[i]:offs[i + 1]]) for i, (e0, e1) in enumerate(ranges)]
    return msg, msg[:hb].view(torch.float32)[:nseg], parts


def qsgd_norms(x, xhat=None, seg_off=None, nseg=1, gossip=None, out=None):
    """The QSGD norm pass alone (per-segment ||x - xhat||_2, fp64, rounded once);
    `gossip=(memory, gamma)` applies the consensus step to x in the same pass."""
    _require(x, torch.float32, "x")
    if xhat is not None:
        _require(xhat, torch.float32, "xhat")
    dev = x.device
    norms = out if out is not None else torch.empty(nseg, dtype=torch.float32, device=dev)
    _require(norms, torch.float32, "norms")
    L = lib()
    ws = workspace(dev, "acc", L.choco_qsgd_workspace_size(nseg))
    g = _gossip(gossip, x, xhat)
    if g is not None:
        _lib.check(L.choco_gossip_qsgd_norms(_ptr(x), _ptr(g[0]), _ptr(xhat), g[1], x.numel(), _ptr(seg_off),
                                             int(nseg), _ptr(norms), _ptr(ws), ws.numel(), _stream(dev)),
                   "choco_gossip_qsgd_norms")
    else:
        _lib.check(L.choco_qsgd_norms(_ptr(x), _ptr(xhat), x.numel(), _ptr(seg_off), int(nseg), _ptr(norms),
                                      _ptr(ws), ws.numel(), _stream(dev)), "choco_qsgd_norms")
    return norms


def qsgd_recv_gossip_norms(messages, weights, self_slot, x, memory, xhat, gamma, q, is_biased=False, seg_off=None,
                           nseg=1, out=None):
    """The deferred receive fused into the next step's first pass (include/choco_codec.h
    choco_qsgd_recv_gossip_norms): the previous step's messages [(packed, norms)] into x_hat
    (self_slot) and memory in order, then x += gamma (memory - x_hat), then this step's
    per-segment norms of x - x_hat (returned, or written to `out`).  More than 8 messages:
    the leading chunks are applied by qsgd_accumulate first (same order, same results)."""
    _require(x, torch.float32, "x")
    _require(xhat, torch.float32, "xhat")
    _check_layout(memory, xhat, x.numel(), seg_off, nseg)
    n = x.numel()
    if len(messages) != len(weights) or not messages:
        raise RuntimeError("one weight per message, at least one message")
    head = max(0, len(messages) - MAX_FUSED_MSGS)  # leading messages: applied first, in order
    (pp, nn, ww, m, slot, _keep), = _msg_tables(messages[head:], weights[head:], self_slot - head, torch.uint8, "QSGD",
                                                qsgd_packed_bytes(n, q), "bytes", nseg)
    dev = x.device
    norms = out if out is not None else torch.empty(nseg, dtype=torch.float32, device=dev)
    _require(norms, torch.float32, "norms")
    if head > 0:
        qsgd_accumulate(messages[:head], weights[:head], self_slot, n, q, memory, xhat_self=xhat,
                        is_biased=is_biased, seg_off=seg_off, nseg=nseg)
    L = lib()
    ws = workspace(dev, "acc", L.choco_qsgd_workspace_size(nseg))
    _lib.check(L.choco_qsgd_recv_gossip_norms(pp, nn, ww, m, slot, _ptr(x), _ptr(memory), _ptr(xhat),
                                              float(gamma), n, _ptr(seg_off), int(nseg), int(q),
                                              1 if is_biased else 0, _ptr(norms), _ptr(ws), ws.numel(),
                                              _stream(dev)), "choco_qsgd_recv_gossip_norms")
    return norms


def qsgd_quantize_range(x, q, norms, e0, e1, packed_range, is_biased=False, xhat=None, seg_off=None, nseg=1,
                        seed=0, offset=0):
    """Quantize elements [e0, e1) into `packed_range` (qsgd_packed_bytes(e1 - e0, q) bytes)."""
    _require(x, torch.float32, "x")
    _require(norms, torch.float32, "norms")
    _require(packed_range, torch.uint8, "packed_range")
    if packed_range.numel() != qsgd_packed_bytes(e1 - e0, q):
        raise RuntimeError("packed_range must hold qsgd_packed_bytes(e1 - e0, q) bytes")
    _lib.check(lib().choco_qsgd_quantize_range(_ptr(x), _ptr(xhat), x.numel(), _ptr(seg_off), int(nseg), int(q),
                                               1 if is_biased else 0, _ptr(norms), int(seed) & (2**64 - 1),
                                               int(offset) & (2**64 - 1), int(e0), int(e1), _ptr(packed_range),
                                               _stream(x.device)), "choco_qsgd_quantize_range")


def qsgd_accumulate_range(messages, weights, self_slot, n, q, memory, e0, e1, xhat_self=None, is_biased=False,
                          seg_off=None, nseg=1):
    """qsgd_accumulate over elements [e0, e1); messages: list of (range message, norms)."""
    _require(memory, torch.float32, "memory")
    _check_layout(memory, xhat_self, n, seg_off, nseg)
    for pp, nn, ww, m, slot, _keep in _msg_tables(messages, weights, self_slot, torch.uint8, "QSGD range",
                                                  qsgd_packed_bytes(e1 - e0, q), "bytes", nseg):
        _lib.check(lib().choco_qsgd_decompress_accumulate_range(
            pp, nn, ww, m, slot, int(n), _ptr(seg_off), int(nseg), int(q), 1 if is_biased else 0, int(e0),
            int(e1), _ptr(xhat_self if slot >= 0 else None), _ptr(memory), _stream(memory.device)),
            "choco_qsgd_decompress_accumulate_range")


def qsgd_extrapolate(packed, norms, n, q, target, a, b, is_biased=False, seg_off=None, nseg=1):
    """target = fmaf(b, decode(m), target * a): ECD (ecd_psgd.py:415-423)."""
    _require(packed, torch.uint8, "packed")
    _require(norms, torch.float32, "norms")
    _require(target, torch.float32, "target")
    _check_layout(target, None, n, seg_off, nseg)
    _lib.check(lib().choco_qsgd_decompress_extrapolate(_ptr(packed), _ptr(norms), int(n), _ptr(seg_off), int(nseg),
                                                       int(q), 1 if is_biased else 0, float(a), float(b),
                                                       _ptr(target), _stream(target.device)),
               "choco_qsgd_decompress_extrapolate")


# ----------------------------------------------------------------------------- gossip
def gossip_step(x, memory, xhat, gamma):
    for t, nm in ((x, "x"), (memory, "memory"), (xhat, "xhat")):
        _require(t, torch.float32, nm)
    _lib.check(lib().choco_gossip_step(_ptr(x), _ptr(memory), _ptr(xhat), float(gamma), x.numel(),
                                       _stream(x.device)), "choco_gossip_step")


# ----------------------------------------------------------------------------- parameter bridge
PARAM_DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}  # CHOCO_DT_*


def params_launches(nseg):
    """Launches one params_pack / params_unpack of `nseg` tensors takes."""
    return int(lib().choco_params_launches(int(nseg)))


def _param_tables(tensors, flat):
    _require(flat, torch.float32, "flat")
    nseg = len(tensors)
    ptrs, lens, dts = (ctypes.c_void_p * nseg)(), (ctypes.c_int64 * nseg)(), (ctypes.c_int32 * nseg)()
    for i, t in enumerate(tensors):
        if not isinstance(t, torch.Tensor) or t.device != flat.device:
            raise RuntimeError(f"tensor {i} must be a torch.Tensor on {flat.device}")
        if not t.is_contiguous():
            raise RuntimeError(f"tensor {i} must be contiguous")
        code = PARAM_DTYPES.get(t.dtype)
        if code is None:
            raise RuntimeError(f"tensor {i} must be float32, bfloat16 or float16, got {t.dtype}")
        ptrs[i], lens[i], dts[i] = t.data_ptr(), t.numel(), code
    return ptrs, lens, dts, nseg


def params_pack(tensors, flat):
    """flat[off_s : off_s + len_s] = tensors[s] widened to fp32, for every tensor in one batched
    launch per chunk (flatten(), communication.py:58-76).  sum of the lengths == flat.numel()."""
    ptrs, lens, dts, nseg = _param_tables(tensors, flat)
    _lib.check(lib().choco_params_pack(ptrs, lens, dts, nseg, _ptr(flat), flat.numel(), _stream(flat.device)),
               "choco_params_pack")


def _sr_words(sr):
    """sr = (seed, step) as the two uint64 arguments."""
    seed, step = sr
    return int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF


def params_unpack(flat, tensors, sr=None):
    """tensors[s][...] = flat[off_s : off_s + len_s] narrowed to the tensor's dtype (round to
    nearest even, as torch's converting copy), one batched launch per chunk
    (TensorBuffer.unpack, tensor_buffer.py:38-40).

    sr = (seed, step): choco_params_unpack_sr -- a bf16 tensor receives the stochastic rounding
    of its flat values with the bits of (seed, step, flat index) (rounding.sr_bits /
    sr_narrow_bf16 restate it), an fp32 tensor the copy; an fp16 tensor raises."""
    ptrs, lens, dts, nseg = _param_tables(tensors, flat)
    if sr is not None:
        _lib.check(lib().choco_params_unpack_sr(ptrs, lens, dts, nseg, _ptr(flat), flat.numel(), *_sr_words(sr),
                                                _stream(flat.device)), "choco_params_unpack_sr")
        return
    _lib.check(lib().choco_params_unpack(ptrs, lens, dts, nseg, _ptr(flat), flat.numel(), _stream(flat.device)),
               "choco_params_unpack")


# ----------------------------------------------------------------------------- SGD update + pack
SGD_F_NESTEROV, SGD_F_FIRST, SGD_F_NOGRAD = 1, 2, 4                    # CHOCO_SGD_F_*
SGD_MODE_GRAD, SGD_MODE_WRITE_PARAMS, SGD_MODE_WRITE_GRADS = 1, 2, 4   # CHOCO_SGD_MODE_*
SGD_MODE_ADD_FLAT = 8                                                  # choco_params_sgd_clip only
SGD_MODE_WRITE_CLIPPED = 16                                            # choco_params_sgd[_master]_gclip only


def params_sgd_launches(nseg):
    """Launches one params_sgd of `nseg` tensors takes."""
    return int(lib().choco_params_sgd_launches(int(nseg)))


def params_gradnorm_launches(nseg, pinned=False):
    """Launches one ParamSgdPlan.gradnorm of `nseg` tensors takes (pinned: with total_norm)."""
    return int(lib().choco_params_gradnorm_launches(int(nseg), 1 if pinned else 0))


def common_grad_dtype(dtypes):
    """The dtype of clip_grad_norm_'s coefficient for gradients of these dtypes: all bfloat16 ->
    bfloat16, all float16 -> float16, any float32 or any mix (or none) -> float32."""
    kinds = set(dtypes)
    return kinds.pop() if len(kinds) == 1 else torch.float32


class ParamSgdPlan:
    """The host tables of choco_params_sgd for one parameter list, built once: lengths and
    dtype codes are fixed; a step rewrites only what changes -- the data pointers
    (`param_ptrs`, `grad_ptrs`, `buf_ptrs`), `flags` (SGD_F_*) and the hyperparameters
    (`lr`, `weight_decay`, `momentum`, `dampening`, doubles) -- by index, then calls run().
    Holds weak references to the parameters only."""

    def __init__(self, params):
        params = list(params)
        if not params:
            raise RuntimeError("ParamSgdPlan needs at least one parameter")
        nseg = len(params)
        self.nseg, self.device = nseg, params[0].device
        self.param_ptrs, self.grad_ptrs, self.buf_ptrs = ((ctypes.c_void_p * nseg)() for _ in range(3))
        self.lens, self.dts, self.flags = (ctypes.c_int64 * nseg)(), (ctypes.c_int32 * nseg)(), (ctypes.c_int32 * nseg)()
        self.lr, self.weight_decay, self.momentum, self.dampening = ((ctypes.c_double * nseg)() for _ in range(4))
        self.dtypes, self.numels = [], []
        for i, p in enumerate(params):
            _require(p, None, f"param {i}")
            if p.device != self.device:
                raise RuntimeError(f"param {i} is on {p.device}, param 0 on {self.device}")
            code = PARAM_DTYPES.get(p.dtype)
            if code is None:
                raise RuntimeError(f"param {i} must be float32, bfloat16 or float16, got {p.dtype}")
            self.lens[i], self.dts[i] = p.numel(), code
            self.dtypes.append(p.dtype)
            self.numels.append(p.numel())
        self.n = sum(self.numels)
        self.seen = [None] * nseg  # the hyperparameter tuple last written, per tensor
        self._norms = self._norm_ws = None  # sqnorm()'s output and workspace, allocated on first use
        self._gn_out = self._gn_ws = None   # gradnorm()'s
        self._ls_out = None                 # gradnorm_scaled()'s
        self._cons_out = self._cons_ws = None  # consensus()'s
        self._refs = [weakref.ref(p) for p in params]

    def holds(self, params):
        """Whether the plan was built for exactly these tensor objects."""
        return len(params) == self.nseg and all(r() is p for r, p in zip(self._refs, params))

    def fits(self, i, t):
        """Whether tensor t can stand as the gradient or momentum buffer of parameter i."""
        return (t.dtype == self.dtypes[i] and t.device == self.device and t.numel() == self.numels[i]
                and t.is_contiguous())

    def sqnorm(self):
        """One choco_params_sqnorm over the tables as they stand: the per-tensor L2 norms of
        d = g (+ wd * p), what DGC._clip_gradient sees (dgc.py:254-256).  Returns the plan's own
        fp32 tensor of nseg norms (overwritten by the next call)."""
        L = lib()
        if self._norms is None:
            self._norms = torch.empty(self.nseg, dtype=torch.float32, device=self.device)
            self._norm_ws = torch.empty(int(L.choco_params_sqnorm_workspace_size(self.nseg, self.n)),
                                        dtype=torch.uint8, device=self.device)
        _lib.check(L.choco_params_sqnorm(self.param_ptrs, self.grad_ptrs, self.lens, self.dts, self.weight_decay,
                                         self.flags, self.nseg, self.n, _ptr(self._norms), _ptr(self._norm_ws),
                                         self._norm_ws.numel(), _stream(self.device)), "choco_params_sqnorm")
        return self._norms

    def gradnorm(self, max_norm, coef_dtype=None, total_norm=None, norms=None):
        """One choco_params_gradnorm over the gradient pointers and flags as they stand:
        torch.nn.utils.clip_grad_norm_'s total L2 norm over every tensor that has a gradient
        (fp64 accumulation in a fixed order) and its clip coefficient, both left on the device.
        Returns the plan's own two-element fp32 tensor [total, coefficient], overwritten by the
        next call: hand it to run(gclip=...) / run_master(gclip=...).

        coef_dtype: the dtype the coefficient is computed in; default: the common dtype of the
        gradients (common_grad_dtype).  total_norm (a one-element tensor or a float): the total
        is pinned to it -- no norm pass, one launch.  norms (fp32 device tensor of nseg; not
        with total_norm) receives the per-tensor norms, sqnorm()'s at zero weight decay."""
        L = lib()
        if coef_dtype is None:
            coef_dtype = common_grad_dtype(dt for dt, fl in zip(self.dtypes, self.flags) if not fl & SGD_F_NOGRAD)
        cd = PARAM_DTYPES.get(coef_dtype)
        if cd is None:
            raise RuntimeError(f"coef_dtype must be float32, bfloat16 or float16, got {coef_dtype}")
        if self._gn_out is None:
            self._gn_out = torch.empty(2, dtype=torch.float32, device=self.device)
        if total_norm is not None:
            if norms is not None:
                raise RuntimeError("norms with a pinned total_norm: there is no norm pass to take them from")
            if not torch.is_tensor(total_norm):
                total_norm = torch.tensor([float(total_norm)], dtype=torch.float32)
            if total_norm.numel() != 1:
                raise RuntimeError("total_norm must hold one element")
            total_norm = total_norm.detach().reshape(1).to(device=self.device, dtype=torch.float32)
        elif self._gn_ws is None:
            self._gn_ws = torch.empty(int(L.choco_params_gradnorm_workspace_size(self.nseg, self.n)),
                                      dtype=torch.uint8, device=self.device)
        if norms is not None:
            _require(norms, torch.float32, "norms")
            if norms.device != self.device or norms.numel() != self.nseg:
                raise RuntimeError(f"norms must hold {self.nseg} elements on {self.device}")
        ws = None if total_norm is not None else self._gn_ws
        _lib.check(L.choco_params_gradnorm(self.grad_ptrs, self.lens, self.dts, self.flags, self.nseg, self.n,
                                           float(max_norm), cd, _ptr(total_norm), _ptr(self._gn_out), _ptr(norms),
                                           _ptr(ws), 0 if ws is None else ws.numel(), _stream(self.device)),
                   "choco_params_gradnorm")
        return self._gn_out

    def gradnorm_scaled(self, scaler, max_norm=None, coef_dtype=None, norms=None, update_state=True):
        """One choco_params_gradnorm_scaled over the gradient pointers and flags as they stand,
        the gradients still multiplied by the loss scale: gradnorm()'s norm pass, then ONE
        launch that tests the fp64 sum of squares for an inf / NaN, unscales the total, computes
        the clip coefficient (max_norm None: 1) times 1 / scale, and updates `scaler`'s device
        state as torch._amp_update_scale_ does.  scaler: a utils.LossScaler (its `_scale` and
        `_growth_tracker` tensors on this device, and its three factors).  Returns the plan's
        own four-element fp32 tensor [total, coefficient / scale, found, scale], overwritten by
        the next call: hand it to run(scaled=...) / run_master(scaled=...).  Nothing is read on
        the host.  There is no pinned total: it would have no norm pass to detect an overflow
        from.

        update_state=False: choco_params_gradnorm_scaled_local -- the same four floats, the
        scaler's state read and left as it is (the all-reduce step: the ranks agree on `found`
        first, then loss_scale_update moves the state)."""
        L = lib()
        if coef_dtype is None:
            coef_dtype = common_grad_dtype(dt for dt, fl in zip(self.dtypes, self.flags) if not fl & SGD_F_NOGRAD)
        cd = PARAM_DTYPES.get(coef_dtype)
        if cd is None:
            raise RuntimeError(f"coef_dtype must be float32, bfloat16 or float16, got {coef_dtype}")
        scale, tracker = scaler._scale, scaler._growth_tracker
        _require(scale, torch.float32, "the loss scale")
        _require(tracker, torch.int32, "the growth tracker")
        if scale.device != self.device or tracker.device != self.device or scale.numel() != 1 or tracker.numel() != 1:
            raise RuntimeError(f"the loss scaler's state must be one-element tensors on {self.device}")
        if self._ls_out is None:
            self._ls_out = torch.empty(4, dtype=torch.float32, device=self.device)
        if self._gn_ws is None:
            self._gn_ws = torch.empty(int(L.choco_params_gradnorm_workspace_size(self.nseg, self.n)),
                                      dtype=torch.uint8, device=self.device)
        if norms is not None:
            _require(norms, torch.float32, "norms")
            if norms.device != self.device or norms.numel() != self.nseg:
                raise RuntimeError(f"norms must hold {self.nseg} elements on {self.device}")
        name = "choco_params_gradnorm_scaled" if update_state else "choco_params_gradnorm_scaled_local"
        _lib.check(getattr(L, name)(self.grad_ptrs, self.lens, self.dts, self.flags, self.nseg, self.n,
                                    0.0 if max_norm is None else float(max_norm), cd, _ptr(scale), _ptr(tracker),
                                    float(scaler.growth_factor), float(scaler.backoff_factor),
                                    int(scaler.growth_interval), 0 if max_norm is None else 1, _ptr(self._ls_out),
                                    _ptr(norms), _ptr(self._gn_ws), self._gn_ws.numel(), _stream(self.device)), name)
        return self._ls_out

    def loss_scale_update(self, scaler, gsum):
        """One choco_loss_scale_update: `gsum` (fp32, n + 1 elements) is the flat buffer after
        the all-reduce, its last element the sum of the ranks' overflow flags.  scaler.last
        (gradnorm_scaled(update_state=False)'s tensor) receives the common flag in its third
        element, and the scaler's device state is backed off or grown as
        torch._amp_update_scale_ does.  One launch; nothing is read on the host."""
        _require(gsum, torch.float32, "gsum")
        if gsum.device != self.device or gsum.numel() != self.n + 1:
            raise RuntimeError(f"gsum must hold {self.n + 1} elements on {self.device}")
        out, scale, tracker = scaler.last, scaler._scale, scaler._growth_tracker
        if out is None:
            raise RuntimeError("loss_scale_update needs scaler.last, gradnorm_scaled(update_state=False)'s tensor")
        _require(out, torch.float32, "scaler.last")
        _require(scale, torch.float32, "the loss scale")
        _require(tracker, torch.int32, "the growth tracker")
        if any(t.device != self.device for t in (out, scale, tracker)) or out.numel() != 4 or scale.numel() != 1 \
                or tracker.numel() != 1:
            raise RuntimeError(f"the loss scaler's state and `last` must be tensors of 1, 1 and 4 elements on "
                               f"{self.device}")
        _lib.check(lib().choco_loss_scale_update(gsum.data_ptr() + 4 * self.n, _ptr(scale), _ptr(tracker),
                                                 float(scaler.growth_factor), float(scaler.backoff_factor),
                                                 int(scaler.growth_interval), _ptr(out), _stream(self.device)),
                   "choco_loss_scale_update")

    def _scaled_ptr(self, scaled, others):
        """scaled (gradnorm_scaled()'s tensor) as a pointer; `others`: whether a keyword it does
        not combine with was given."""
        if others:
            raise RuntimeError("scaled (the loss-scaled step) does not combine with gclip, norms / clip_threshold / "
                               "add_flat or grad_mode: its clip is gradnorm_scaled(max_norm=)'s")
        _require(scaled, torch.float32, "scaled")
        if scaled.device != self.device or scaled.numel() != 4:
            raise RuntimeError(f"scaled must be gradnorm_scaled()'s four-element tensor on {self.device}")
        return scaled.data_ptr()

    def _coef_ptr(self, gclip):
        _require(gclip, torch.float32, "gclip")
        if gclip.device != self.device or gclip.numel() != 2:
            raise RuntimeError(f"gclip must be gradnorm()'s two-element tensor on {self.device}")
        return gclip.data_ptr() + 4

    def _sgd(self, variant, *tail):
        """One call of the entry point choco_params_sgd<variant>: the eleven table arguments as
        they stand, then `tail`, then the stream."""
        name = "choco_params_sgd" + variant
        _lib.check(getattr(lib(), name)(self.param_ptrs, self.grad_ptrs, self.buf_ptrs, self.lens, self.dts, self.lr,
                                        self.weight_decay, self.momentum, self.dampening, self.flags, self.nseg,
                                        *tail, _stream(self.device)), name)

    def run(self, flat=None, grad_mode=False, write=True, norms=None, clip_threshold=None, add_flat=False,
            gclip=None, write_clipped=False, scaled=None, sr=None):
        """One choco_params_sgd over the tables as they stand.  apply mode (grad_mode False):
        write -> the params are updated; grad mode: write -> d_p goes into the grads' storage.
        flat (fp32, n elements, or None) receives the new params / d_p in the same pass.

        norms (fp32 device tensor of nseg, e.g. sqnorm()'s) with clip_threshold (a Python float,
        clip_grad_val / sqrt(n_nodes)): DGC's per-tensor clipping between the weight decay and
        the momentum; add_flat (grad mode): flat += d_p instead of flat = d_p.  Either one takes
        choco_params_sgd_clip; the defaults are choco_params_sgd, as before.

        gclip (gradnorm()'s tensor): choco_params_sgd_gclip -- every gradient is scaled by the
        global-norm clip coefficient as it is loaded; write_clipped (apply mode): the clipped
        gradient is also stored into the grads' storage.  Not together with norms /
        clip_threshold / add_flat.

        scaled (gradnorm_scaled()'s tensor; apply mode, none of the keywords above):
        choco_params_sgd_scaled -- every gradient is multiplied by its second element (the clip
        coefficient over the loss scale), and where its third says the gradients held an inf or
        a NaN the step is skipped on the device: flat receives the unchanged params and nothing
        else is written.  write_clipped stores the unscaled, clipped gradient.

        sr = (seed, step) (apply mode; bf16 and fp32 tensors; with or without gclip /
        write_clipped): choco_params_sgd_sr -- the parameter line stays fp32, flat receives
        p_new unrounded and a bf16 parameter, where written, its stochastic rounding with the
        bits of (seed, step, flat index).  Not with grad_mode, norms / clip_threshold /
        add_flat or scaled."""
        if flat is not None:
            _require(flat, torch.float32, "flat")
            if flat.device != self.device or flat.numel() != self.n:
                raise RuntimeError(f"flat must hold {self.n} elements on {self.device}")
        mode = (SGD_MODE_GRAD | (SGD_MODE_WRITE_GRADS if write else 0)) if grad_mode else \
            (SGD_MODE_WRITE_PARAMS if write else 0)
        clipped = SGD_MODE_WRITE_CLIPPED if write_clipped else 0
        if sr is not None:
            if scaled is not None:
                raise RuntimeError("sr (stochastic rounding) has no loss-scaled form: bf16 needs no loss scale, "
                                   "and fp16 models use LossScaler with MasterWeights")
            if norms is not None or clip_threshold is not None:
                raise RuntimeError("sr (stochastic rounding) does not combine with norms / clip_threshold (DGC's "
                                   "per-tensor clipping)")
            if gclip is None and write_clipped:
                raise RuntimeError("write_clipped needs gclip (gradnorm()'s tensor)")
            # grad mode and add_flat are refused by the entry point, with its own messages
            mode |= SGD_MODE_ADD_FLAT if add_flat else 0
            return self._sgd("_sr", _ptr(flat), self.n, mode | clipped,
                             None if gclip is None else self._coef_ptr(gclip), *_sr_words(sr))
        if scaled is not None:
            out = self._scaled_ptr(scaled, gclip is not None or norms is not None or clip_threshold is not None
                                   or add_flat or grad_mode)
            return self._sgd("_scaled", _ptr(flat), self.n, mode | clipped, out)
        if gclip is None and write_clipped:
            raise RuntimeError("write_clipped needs gclip (gradnorm()'s tensor)")
        if gclip is not None:
            if norms is not None or clip_threshold is not None or add_flat:
                raise RuntimeError("gclip (global-norm clipping) does not combine with norms / clip_threshold / "
                                   "add_flat (DGC's per-tensor clipping)")
            if write_clipped and grad_mode:
                raise RuntimeError("write_clipped is for apply mode: grad mode writes d_p into the grads")
            return self._sgd("_gclip", _ptr(flat), self.n, mode | clipped, self._coef_ptr(gclip))
        if clip_threshold is not None and norms is None:
            raise RuntimeError("clip_threshold needs norms (sqnorm()'s, or recorded ones): nothing would be clipped")
        if norms is not None or add_flat:
            if norms is not None:
                _require(norms, torch.float32, "norms")
                if norms.device != self.device or norms.numel() != self.nseg:
                    raise RuntimeError(f"norms must hold {self.nseg} elements on {self.device}")
                if clip_threshold is None:
                    raise RuntimeError("norms needs a clip_threshold")
            return self._sgd("_clip", _ptr(flat), self.n, mode | (SGD_MODE_ADD_FLAT if add_flat else 0), _ptr(norms),
                             float(clip_threshold) if norms is not None else 0.0)
        self._sgd("", _ptr(flat), self.n, mode)

    def fits_master_buf(self, i, t):
        """Whether tensor t can stand as the fp32 momentum buffer of parameter i in a master
        update (the buffers are fp32 whatever the parameter's dtype)."""
        return (t.dtype == torch.float32 and t.device == self.device and t.numel() == self.numels[i]
                and t.is_contiguous())

    def run_master(self, master, write=True, gclip=None, write_clipped=False, scaled=None):
        """One choco_params_sgd_master over the tables as they stand: the update runs on
        `master` (the persistent flat fp32 copy of the parameters, n elements) in place, with
        fp32 momentum buffers behind `buf_ptrs` and the gradients in their parameters' dtype;
        write -> the parameters receive the new master values narrowed to their dtype.

        gclip (gradnorm(coef_dtype=torch.float32)'s tensor): choco_params_sgd_master_gclip --
        g = c * g in fp32, not narrowed, in front of the update; write_clipped: that product,
        narrowed, is stored into the grads' storage.

        scaled (gradnorm_scaled(coef_dtype=torch.float32)'s tensor; not with gclip):
        choco_params_sgd_master_scaled -- the same with its second element as the coefficient,
        and a step its third element marks as overflowed touches nothing."""
        _require(master, torch.float32, "master")
        if master.device != self.device or master.numel() != self.n:
            raise RuntimeError(f"master must hold {self.n} elements on {self.device}")
        mode = (SGD_MODE_WRITE_PARAMS if write else 0) | (SGD_MODE_WRITE_CLIPPED if write_clipped else 0)
        if scaled is not None:
            return self._sgd("_master_scaled", _ptr(master), self.n, mode, self._scaled_ptr(scaled, gclip is not None))
        if gclip is None and write_clipped:
            raise RuntimeError("write_clipped needs gclip (gradnorm()'s tensor)")
        if gclip is not None:
            return self._sgd("_master_gclip", _ptr(master), self.n, mode, self._coef_ptr(gclip))
        self._sgd("_master", _ptr(master), self.n, mode)

    def pack_grads(self, flat, coef=None, found=None, round=True):
        """One choco_params_pack of the gradients behind `grad_ptrs` as they stand into `flat`
        (fp32, n elements), widening 16-bit gradients (exact): TensorBuffer(grads) of
        sgd.py:71-74 with no table built per step.

        coef (gradnorm()'s two-element or gradnorm_scaled()'s four-element tensor):
        choco_params_pack_scaled -- every gradient is multiplied by its second element on the
        load; round (default) narrows the product once to the gradient's dtype, as the gclip /
        scaled update kernels do, round=False leaves the fp32 product (the master path).
        found (gradnorm_scaled()'s tensor; needs coef): flat holds n + 1 elements and the last
        receives 1.0 where its third element is not zero, else 0.0."""
        _require(flat, torch.float32, "flat")
        if found is not None and coef is None:
            raise RuntimeError("pack_grads: found needs coef")
        want = self.n + (0 if found is None else 1)
        if flat.device != self.device or flat.numel() != want:
            raise RuntimeError(f"flat must hold {want} elements on {self.device}")
        if coef is None:
            _lib.check(lib().choco_params_pack(self.grad_ptrs, self.lens, self.dts, self.nseg, _ptr(flat), self.n,
                                               _stream(self.device)), "choco_params_pack")
            return
        _require(coef, torch.float32, "coef")
        if coef.device != self.device or coef.numel() not in (2, 4):
            raise RuntimeError(f"coef must be gradnorm()'s or gradnorm_scaled()'s tensor on {self.device}")
        f_ptr = None
        if found is not None:
            _require(found, torch.float32, "found")
            if found.device != self.device or found.numel() != 4:
                raise RuntimeError(f"found must be gradnorm_scaled()'s four-element tensor on {self.device}")
            f_ptr = found.data_ptr() + 8
        _lib.check(lib().choco_params_pack_scaled(self.grad_ptrs, self.lens, self.dts, self.nseg, _ptr(flat), self.n,
                                                  coef.data_ptr() + 4, f_ptr, 1 if round else 0,
                                                  _stream(self.device)), "choco_params_pack_scaled")

    def run_flatgrad(self, gsum, divisor, write=True, write_grads=True, master=None, found_slot=False):
        """One choco_params_sgd_flatgrad (master: choco_params_sgd_master_flatgrad) over the
        tables as they stand: the update whose gradient is gsum / divisor, gsum the flat fp32
        buffer of the all-reduced gradient sum (n elements).  write -> the params are written;
        write_grads -> the averaged gradient goes into the storage behind `grad_ptrs`, narrowed
        to the tensor's dtype.  master (flat fp32, n elements): the update runs on it in place
        with fp32 momentum buffers and the unrounded average.

        found_slot: choco_params_sgd[_master]_flatgrad_scaled -- gsum holds n + 1 elements, and
        where the last (the all-reduced sum of the ranks' overflow flags) is not zero the step
        is skipped on the device: nothing is written."""
        _require(gsum, torch.float32, "gsum")
        want = self.n + (1 if found_slot else 0)
        if gsum.device != self.device or gsum.numel() != want:
            raise RuntimeError(f"gsum must hold {want} elements on {self.device}")
        tail = "_scaled" if found_slot else ""
        mode = (SGD_MODE_WRITE_PARAMS if write else 0) | (SGD_MODE_WRITE_GRADS if write_grads else 0)
        if master is None:
            return self._sgd("_flatgrad" + tail, _ptr(gsum), self.n, float(divisor), mode)
        _require(master, torch.float32, "master")
        if master.device != self.device or master.numel() != self.n:
            raise RuntimeError(f"master must hold {self.n} elements on {self.device}")
        self._sgd("_master_flatgrad" + tail, _ptr(gsum), _ptr(master), self.n, float(divisor), mode)

    def mix(self, srcs, weights, lr=0.0, mode=0, ext_a=0.0, ext_b=0.0, flat_out=None, x_out=None):
        """One choco_params_mix over the plan's parameter and gradient pointers as they stand
        (params_mix describes the arguments)."""
        _mix_call(srcs, weights, self.param_ptrs, self.grad_ptrs, self.lens, self.dts, self.nseg, self.n, self.device,
                  lr, mode, ext_a, ext_b, flat_out, x_out)

    def ef(self, flat, mode, lr=0.0, divisor=1.0):
        """One choco_params_ef over the plan's parameter pointers as they stand (params_ef
        describes the arguments)."""
        _ef_call(self.param_ptrs, self.lens, self.dts, self.nseg, self.n, self.device, flat, mode, lr, divisor)

    def consensus(self, xsum, divisor, avg_out=None, master=None, dists=None, want_dist=True):
        """One choco_params_consensus over the plan's parameter pointers as they stand
        (params_consensus describes the arguments).  The workspace and the two-element fp32
        output are the plan's own, allocated on first use; returns that output (overwritten by
        the next call), or None without want_dist."""
        L = lib()
        for name, t in (("xsum", xsum), ("master", master)):
            if t is None and name == "master":
                continue
            _require(t, torch.float32, name)
            if t.device != self.device or t.numel() != self.n:
                raise RuntimeError(f"{name} must hold {self.n} elements on {self.device}")
        mode = (CONS_DIST if want_dist else 0) | (CONS_WRITE_AVG if avg_out is not None else 0)
        if not mode:
            raise RuntimeError("params_consensus: nothing to do without want_dist and avg_out")
        avg_ptrs = None
        if avg_out is not None:
            avg_out = list(avg_out)
            if len(avg_out) != self.nseg:
                raise RuntimeError(f"avg_out: {len(avg_out)} tensors for {self.nseg} parameters")
            avg_ptrs = (ctypes.c_void_p * self.nseg)()
            for i, t in enumerate(avg_out):
                if not isinstance(t, torch.Tensor) or not self.fits(i, t):
                    raise RuntimeError(f"avg_out {i} must match its parameter's dtype, device and size, and be "
                                       "contiguous")
                avg_ptrs[i] = t.data_ptr()
        out = ws = None
        if want_dist:
            if self._cons_out is None:
                self._cons_out = torch.empty(2, dtype=torch.float32, device=self.device)
                self._cons_ws = torch.empty(int(L.choco_params_consensus_workspace_size(self.nseg, self.n)),
                                            dtype=torch.uint8, device=self.device)
            out, ws = self._cons_out, self._cons_ws
            if dists is not None:
                _require(dists, torch.float32, "dists")
                if dists.device != self.device or dists.numel() != self.nseg:
                    raise RuntimeError(f"dists must hold {self.nseg} elements on {self.device}")
        elif dists is not None:
            raise RuntimeError("dists without want_dist")
        _lib.check(L.choco_params_consensus(self.param_ptrs, avg_ptrs, self.lens, self.dts, self.nseg, _ptr(xsum),
                                            _ptr(master), self.n, float(divisor), mode, _ptr(out), _ptr(dists),
                                            _ptr(ws), 0 if ws is None else ws.numel(), _stream(self.device)),
                   "choco_params_consensus")
        return out


# ----------------------------------------------------------------------------- consensus evaluation
CONS_DIST, CONS_WRITE_AVG = 1, 2  # CHOCO_CONS_*


def params_consensus_launches(nseg, want_dist=True):
    """Launches one params_consensus over `nseg` tensors takes: one per chunk of tensors and,
    with want_dist, the total launch (writing the averaged model adds none)."""
    return int(lib().choco_params_consensus_launches(int(nseg), CONS_DIST if want_dist else CONS_WRITE_AVG))


def params_consensus(params, xsum, divisor, avg_out=None, master=None, dists=None, want_dist=True, plan=None):
    """The averaged model and this worker's distance to it from the all-reduced SUM of the packed
    parameters, one batched launch per chunk of tensors plus one total launch
    (include/choco_codec.h, choco_params_consensus): per element a = xsum / divisor (a true
    division), d = a - x with x the parameter widened (or master's value: master is the flat fp32
    copy of the parameters), and
        want_dist: out = [sqrt(sum d^2), sqrt(sum a^2)], fp64 sums in a fixed order, rounded once;
                   dists (fp32 device tensor of nseg) receives the per-tensor sqrt(sum d^2);
        avg_out:   a list of tensors matching the parameters; avg_out[s] = a narrowed to its
                   dtype.  It may hold the parameters themselves (agg_model in place): the
                   distance is then that of the values from before the call.
    params: tensors laid out back to back in xsum.  Returns (out, plan): out the plan's own
    two-element device tensor, overwritten by the plan's next call (None without want_dist);
    pass the plan back in to reuse its tables, workspace and output."""
    params = list(params)
    if plan is None:
        plan = ParamSgdPlan(params)
    elif not plan.holds(params):
        raise RuntimeError("the plan was built for another parameter list")
    for i, p in enumerate(params):
        if not p.is_contiguous():
            raise RuntimeError(f"param {i} must be contiguous")
        plan.param_ptrs[i] = p.data_ptr()
    return plan.consensus(xsum, divisor, avg_out, master, dists, want_dist), plan


# ----------------------------------------------------------------------------- neighbour-weighted mix
MIX_GRAD_SUB, MIX_GRAD_FMA, MIX_WRITE_PARAMS, MIX_EXTRAPOLATE = 1, 2, 4, 8  # CHOCO_MIX_*


def params_mix_launches(nseg, nsrc):
    """Launches one params_mix of `nsrc` sources over `nseg` tensors takes."""
    return int(lib().choco_params_mix_launches(int(nseg), int(nsrc)))


def _mix_call(srcs, weights, param_ptrs, grad_ptrs, lens, dts, nseg, n, dev, lr, mode, ext_a, ext_b, flat_out, x_out):
    srcs = list(srcs)
    nsrc = len(srcs)
    if len(weights) != nsrc:
        raise RuntimeError(f"params_mix: {len(weights)} weights for {nsrc} sources")
    named = [(f"source {r}", t) for r, t in enumerate(srcs)]
    named += [(name, t) for name, t in (("flat_out", flat_out), ("x_out", x_out)) if t is not None]
    for name, t in named:
        _require(t, torch.float32, name)
        if t.device != dev or t.numel() != n:
            raise RuntimeError(f"{name} must hold {n} elements on {dev}")
    src_ptrs = (ctypes.c_void_p * max(nsrc, 1))(*[t.data_ptr() for t in srcs])
    w = (ctypes.c_double * max(nsrc, 1))(*[float(v) for v in weights])
    _lib.check(lib().choco_params_mix(src_ptrs, w, nsrc, param_ptrs, grad_ptrs, lens, dts, nseg, float(lr),
                                      float(ext_a), float(ext_b), int(mode), _ptr(flat_out), _ptr(x_out), n,
                                      _stream(dev)), "choco_params_mix")


def params_mix(srcs, weights, params=None, grads=None, lr=0.0, mode=0, ext_a=0.0, ext_b=0.0, flat_out=None,
               x_out=None, plan=None):
    """The neighbour-weighted model mix sum(src_r * w_r) with the tail one of the reference's
    optimizers puts behind it, one batched launch per chunk of tensors (include/choco_codec.h,
    choco_params_mix): m = 0 + src_0 * w_0, m += src_r * w_r in the given order (srcs: flat fp32
    tensors of one size, 1 to 64 of them; weights: Python floats), then
        MIX_GRAD_SUB: m -= lr * grads (two roundings, dcd_psgd.py:124) or
        MIX_GRAD_FMA: m.add_(grads, alpha=-lr) (fused, ecd_psgd.py:131-133);
        MIX_WRITE_PARAMS: params = m (the unpack); MIX_EXTRAPOLATE: flat_out = ext_a * old
        params + ext_b * m in place of m; x_out = the old params, packed.
    params / grads: lists of tensors laid out back to back in the flat buffers (None: the
    sources are mixed as one flat tensor into flat_out).  Returns the plan (pass it back in to
    reuse its tables)."""
    srcs = list(srcs)
    if not srcs:
        raise RuntimeError("params_mix needs at least one source")
    if params is None:
        if grads is not None:
            raise RuntimeError("params_mix: grads without params")
        n = srcs[0].numel()
        lens, dts = (ctypes.c_int64 * 1)(n), (ctypes.c_int32 * 1)(0)
        _mix_call(srcs, weights, None, None, lens, dts, 1, n, srcs[0].device, lr, mode, ext_a, ext_b, flat_out, x_out)
        return None
    params = list(params)
    if plan is None:
        plan = ParamSgdPlan(params)
    elif not plan.holds(params):
        raise RuntimeError("the plan was built for another parameter list")
    grads = _per_tensor(grads, plan.nseg, "grads")
    for i, (p, g) in enumerate(zip(params, grads)):
        if g is not None and not plan.fits(i, g):
            raise RuntimeError(f"grad {i} must match its parameter's dtype, device and size, and be contiguous")
        plan.param_ptrs[i] = p.data_ptr()
        plan.grad_ptrs[i] = g.data_ptr() if g is not None else None
    plan.mix(srcs, weights, lr, mode, ext_a, ext_b, flat_out, x_out)
    return plan


# ----------------------------------------------------------------------------- error-feedback lines
EF_ACCUM, EF_APPLY, EF_DIV, EF_SCALE = 1, 2, 4, 8  # CHOCO_EF_*


def params_ef_launches(nseg):
    """Launches one params_ef over `nseg` tensors takes."""
    return int(lib().choco_params_ef_launches(int(nseg)))


def _ef_call(param_ptrs, lens, dts, nseg, n, dev, flat, mode, lr, divisor):
    _require(flat, torch.float32, "flat")
    if flat.device != dev or flat.numel() != n:
        raise RuntimeError(f"flat must hold {n} elements on {dev}")
    _lib.check(lib().choco_params_ef(param_ptrs, lens, dts, nseg, _ptr(flat), n, int(mode), float(lr), float(divisor),
                                     _stream(dev)), "choco_params_ef")


def params_ef(params, flat, mode, lr=0.0, divisor=1.0, plan=None):
    """The dense lines around the compressors of the two error-feedback optimizers, straight
    between the parameter tensors and a flat fp32 buffer, one batched launch per chunk of
    tensors (include/choco_codec.h, choco_params_ef):
        EF_ACCUM: flat += params (the pack and memory.buffer += params_tb.buffer,
                  deep_squeeze.py:101-108); the params are read only.
        EF_APPLY: params += flat, narrowed once (deep_squeeze.py:125-126), after
            | EF_DIV:   flat /= divisor, a true division, written back (ef_sign_sgd.py:218)
            | EF_SCALE: the addend is (-lr) * flat, not written back (ef_sign_sgd.py:119).
    params: tensors laid out back to back in flat.  Returns the plan (pass it back in to reuse
    its tables)."""
    params = list(params)
    if plan is None:
        plan = ParamSgdPlan(params)
    elif not plan.holds(params):
        raise RuntimeError("the plan was built for another parameter list")
    for i, p in enumerate(params):
        if not p.is_contiguous():
            raise RuntimeError(f"param {i} must be contiguous")
        plan.param_ptrs[i] = p.data_ptr()
    plan.ef(flat, mode, lr, divisor)
    return plan


def _per_tensor(v, nseg, name):
    if isinstance(v, (list, tuple)):
        if len(v) != nseg:
            raise RuntimeError(f"{name}: {len(v)} values for {nseg} tensors")
        return v
    return [v] * nseg


def params_sgd(params, grads, bufs, lr, weight_decay=0.0, momentum=0.0, dampening=0.0, nesterov=False, first=False,
               flat=None, grad_mode=False, write=True, plan=None):
    """apply_gradient (optim/utils.py:13-47) over a list of tensors in one batched launch per
    chunk (include/choco_codec.h, choco_params_sgd).  grads[s] None: p.grad is None (apply mode:
    the tensor is only packed into `flat`).  bufs[s]: the momentum buffer, written when
    momentum != 0 and read unless first[s].  The hyperparameters, `nesterov` and `first` are
    scalars or per-tensor lists.  Returns the plan (pass it back in to reuse its tables)."""
    plan = _sgd_tables(params, grads, bufs, lr, weight_decay, momentum, dampening, nesterov, first, plan, False)
    plan.run(flat, grad_mode, write)
    return plan


def params_sgd_master_launches(nseg):
    """Launches one params_sgd_master of `nseg` tensors takes."""
    return int(lib().choco_params_sgd_master_launches(int(nseg)))


def params_sgd_master(params, grads, bufs, lr, weight_decay=0.0, momentum=0.0, dampening=0.0, nesterov=False,
                      first=False, master=None, write=True, plan=None):
    """apply_gradient on fp32 master weights (include/choco_codec.h, choco_params_sgd_master):
    params_sgd's arguments, except that the update runs in place on `master` -- the persistent
    flat fp32 copy of `params`, laid out back to back -- and bufs[s] is an fp32 tensor whatever
    its parameter's dtype.  grads[s] has its parameter's dtype; None: the tensor is passed over.
    write: the parameters receive the new master values narrowed to their dtype.  Returns the
    plan (pass it back in to reuse its tables)."""
    if master is None:
        raise RuntimeError("params_sgd_master needs the master buffer")
    plan = _sgd_tables(params, grads, bufs, lr, weight_decay, momentum, dampening, nesterov, first, plan, True)
    plan.run_master(master, write)
    return plan


def params_sgd_flatgrad_launches(nseg):
    """Launches one params_sgd_flatgrad of `nseg` tensors takes (with or without master)."""
    return int(lib().choco_params_sgd_flatgrad_launches(int(nseg)))


def params_sgd_flatgrad(params, grads, bufs, gsum, divisor, lr, weight_decay=0.0, momentum=0.0, dampening=0.0,
                        nesterov=False, first=False, master=None, write=True, write_grads=True, plan=None,
                        found_slot=False):
    """The all-reduce SGD update (sgd.py:82-89; include/choco_codec.h, choco_params_sgd_flatgrad
    and choco_params_sgd_master_flatgrad): params_sgd's arguments in apply mode, except that the
    gradient is gsum / divisor -- gsum the flat fp32 buffer of the summed gradients, the tensors
    back to back -- narrowed to each tensor's dtype, and grads[s] is where that averaged gradient
    is written (write_grads; otherwise grads may be None).  master (flat fp32): the update runs
    on it in place with fp32 bufs and the average is not narrowed.  found_slot: gsum holds one
    more element, the all-reduced overflow flag, and anything but zero there skips the step on
    the device (the _scaled entry points).  Returns the plan (pass it back in to reuse its
    tables)."""
    plan = _sgd_tables(params, grads, bufs, lr, weight_decay, momentum, dampening, nesterov, first, plan,
                       master is not None)
    if not write_grads:  # the grads are outputs here: none written, none needed
        for i in range(plan.nseg):
            plan.flags[i] &= ~SGD_F_NOGRAD
    plan.run_flatgrad(gsum, divisor, write, write_grads, master, found_slot)
    return plan


def _sgd_tables(params, grads, bufs, lr, weight_decay, momentum, dampening, nesterov, first, plan, master):
    """The plan of `params` with one call's pointers, flags and hyperparameters written."""
    params = list(params)
    nseg = len(params)
    if plan is None:
        plan = ParamSgdPlan(params)
    elif not plan.holds(params):
        raise RuntimeError("the plan was built for another parameter list")
    cols = [_per_tensor(v, nseg, nm) for v, nm in ((grads, "grads"), (bufs, "bufs"), (lr, "lr"),
                                                   (weight_decay, "weight_decay"), (momentum, "momentum"),
                                                   (dampening, "dampening"), (nesterov, "nesterov"), (first, "first"))]
    for i, (p, g, b, a, wd, mom, damp, nest, fst) in enumerate(zip(params, *cols)):
        if g is not None and not plan.fits(i, g):
            raise RuntimeError(f"grad {i} must match its parameter's dtype, device and size, and be contiguous")
        if b is not None and not (plan.fits_master_buf(i, b) if master else plan.fits(i, b)):
            what = "be float32 and match its parameter's" if master else "match its parameter's dtype,"
            raise RuntimeError(f"buf {i} must {what} device and size, and be contiguous")
        plan.param_ptrs[i] = p.data_ptr()
        plan.grad_ptrs[i] = g.data_ptr() if g is not None else None
        plan.buf_ptrs[i] = b.data_ptr() if b is not None else None
        plan.flags[i] = ((SGD_F_NESTEROV if nest else 0) | (SGD_F_FIRST if fst else 0)
                         | (SGD_F_NOGRAD if g is None else 0))
        plan.lr[i], plan.weight_decay[i], plan.momentum[i], plan.dampening[i] = a, wd, mom, damp
        plan.seen[i] = None
    return plan


ADAM_F_DECOUPLED, ADAM_F_FIRST, ADAM_F_NOGRAD = 1, 2, 4                # CHOCO_ADAM_F_*


def params_adam_launches(nseg):
    """Launches one params_adam / params_adam_master / params_adam(sr=) of `nseg` tensors takes."""
    return int(lib().choco_params_adam_launches(int(nseg)))


class ParamAdamPlan:
    """The host tables of choco_params_adam / choco_params_adam_master for one parameter list,
    built once: a step rewrites only what changes -- the data pointers (`param_ptrs`,
    `grad_ptrs`, `exp_avg_ptrs`, `exp_avg_sq_ptrs`), `flags` (ADAM_F_*), `step` (the count after
    the increment) and the hyperparameters (`lr`, `beta1`, `beta2`, `eps`, `weight_decay`,
    doubles; `seen[i]` is the tuple last written) -- by index, then calls run() / run_master().
    Holds the ParamSgdPlan of the same list (`sgd`) and shares its layout, pointer and flag
    tables: gradnorm() is that plan's, over the gradient pointers and flags as they stand (the
    no-grad bit is the same one)."""

    def __init__(self, params):
        sgd = self.sgd = ParamSgdPlan(params)
        nseg = self.nseg = sgd.nseg
        self.device, self.n, self.dtypes, self.numels = sgd.device, sgd.n, sgd.dtypes, sgd.numels
        self.param_ptrs, self.grad_ptrs, self.flags, self.lr, self.weight_decay = (
            sgd.param_ptrs, sgd.grad_ptrs, sgd.flags, sgd.lr, sgd.weight_decay)
        self.exp_avg_ptrs, self.exp_avg_sq_ptrs = ((ctypes.c_void_p * nseg)() for _ in range(2))
        self.beta1, self.beta2, self.eps, self.step = ((ctypes.c_double * nseg)() for _ in range(4))
        self.seen = [None] * nseg  # the hyperparameter tuple last written, per tensor
        self.holds, self.fits, self.fits_master_buf, self.gradnorm = (sgd.holds, sgd.fits, sgd.fits_master_buf,
                                                                      sgd.gradnorm)

    def _adam(self, name, flat, mode, gclip, write_clipped, sr=()):
        if gclip is None and write_clipped:
            raise RuntimeError("write_clipped needs gclip (gradnorm()'s tensor)")
        sgd = self.sgd
        mode |= SGD_MODE_WRITE_CLIPPED if write_clipped else 0
        _lib.check(getattr(lib(), name)(self.param_ptrs, self.grad_ptrs, self.exp_avg_ptrs, self.exp_avg_sq_ptrs,
                                        sgd.lens, sgd.dts, self.lr, self.beta1, self.beta2, self.eps,
                                        self.weight_decay, self.step, self.flags, self.nseg, _ptr(flat), self.n, mode,
                                        None if gclip is None else sgd._coef_ptr(gclip), *sr, _stream(self.device)),
                   name)

    def run(self, flat=None, write=True, gclip=None, write_clipped=False, sr=None):
        """One choco_params_adam over the tables as they stand: write -> the params are
        updated; flat (fp32, n elements, or None) receives the new params in the same pass (a
        tensor without a gradient is packed as it is).  gclip (gradnorm()'s tensor): every
        gradient is scaled by the global-norm clip coefficient as it is loaded, the product
        narrowed to the tensor's dtype; write_clipped: it is also stored into the grads'
        storage.

        sr = (seed, step): choco_params_adam_sr -- on a bf16 tensor the lines run in fp32 with
        nothing narrowed between them (gclip: coef_dtype=torch.float32's tensor, the product not
        narrowed), exp_avg, exp_avg_sq and, where written, the parameter are stored through the
        stochastic rounding with lanes 1, 2 and 0 of (seed, step, flat index), and flat receives
        p_new unrounded; an fp32 tensor is updated as without; an fp16 tensor raises."""
        if flat is not None:
            _require(flat, torch.float32, "flat")
            if flat.device != self.device or flat.numel() != self.n:
                raise RuntimeError(f"flat must hold {self.n} elements on {self.device}")
        mode = SGD_MODE_WRITE_PARAMS if write else 0
        if sr is not None:
            return self._adam("choco_params_adam_sr", flat, mode, gclip, write_clipped, _sr_words(sr))
        self._adam("choco_params_adam", flat, mode, gclip, write_clipped)

    def run_master(self, master, write=True, gclip=None, write_clipped=False):
        """One choco_params_adam_master over the tables as they stand: the update runs on
        `master` (the persistent flat fp32 copy of the parameters, n elements) in place, with
        fp32 moments behind `exp_avg_ptrs` / `exp_avg_sq_ptrs` and the gradients in their
        parameters' dtype; write -> the parameters receive the new master values narrowed to
        their dtype.  gclip (gradnorm(coef_dtype=torch.float32)'s tensor): g = c * g in fp32,
        not narrowed, in front of the update; write_clipped: that product, narrowed, is stored
        into the grads' storage."""
        _require(master, torch.float32, "master")
        if master.device != self.device or master.numel() != self.n:
            raise RuntimeError(f"master must hold {self.n} elements on {self.device}")
        self._adam("choco_params_adam_master", master, SGD_MODE_WRITE_PARAMS if write else 0, gclip, write_clipped)


def _adam_tables(params, grads, exp_avgs, exp_avg_sqs, lr, betas, eps, weight_decay, step, decoupled, first, plan,
                 master):
    """The plan of `params` with one call's pointers, flags and hyperparameters written."""
    params = list(params)
    nseg = len(params)
    if plan is None:
        plan = ParamAdamPlan(params)
    elif not plan.holds(params):
        raise RuntimeError("the plan was built for another parameter list")
    if isinstance(betas, (tuple, list)) and len(betas) == 2 and not isinstance(betas[0], (list, tuple)):
        betas = [betas] * nseg  # one (beta1, beta2) pair for every tensor
    cols = [_per_tensor(v, nseg, nm) for v, nm in ((grads, "grads"), (exp_avgs, "exp_avgs"),
                                                   (exp_avg_sqs, "exp_avg_sqs"), (lr, "lr"), (betas, "betas"),
                                                   (eps, "eps"), (weight_decay, "weight_decay"), (step, "step"),
                                                   (decoupled, "decoupled"), (first, "first"))]
    for i, (p, g, m, v, a, (b1, b2), e, wd, k, dec, fst) in enumerate(zip(params, *cols)):
        if g is not None and not plan.fits(i, g):
            raise RuntimeError(f"grad {i} must match its parameter's dtype, device and size, and be contiguous")
        for t, nm in ((m, "exp_avg"), (v, "exp_avg_sq")):
            if t is not None and not (plan.fits_master_buf(i, t) if master else plan.fits(i, t)):
                what = "be float32 and match its parameter's" if master else "match its parameter's dtype,"
                raise RuntimeError(f"{nm} {i} must {what} device and size, and be contiguous")
        plan.param_ptrs[i] = p.data_ptr()
        plan.grad_ptrs[i] = g.data_ptr() if g is not None else None
        plan.exp_avg_ptrs[i] = m.data_ptr() if m is not None else None
        plan.exp_avg_sq_ptrs[i] = v.data_ptr() if v is not None else None
        plan.flags[i] = ((ADAM_F_DECOUPLED if dec else 0) | (ADAM_F_FIRST if fst else 0)
                         | (ADAM_F_NOGRAD if g is None else 0))
        plan.lr[i], plan.beta1[i], plan.beta2[i], plan.eps[i], plan.weight_decay[i], plan.step[i] = a, b1, b2, e, wd, k
        plan.seen[i] = None
    return plan


def params_adam(params, grads, exp_avgs, exp_avg_sqs, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1,
                decoupled=False, first=False, flat=None, write=True, gclip=None, write_clipped=False, plan=None,
                sr=None):
    """torch.optim.Adam.step / AdamW.step (decoupled) over a list of tensors in one batched
    launch per chunk (include/choco_codec.h, choco_params_adam).  grads[s] None: p.grad is None
    (the tensor is only packed into `flat`).  exp_avgs[s] / exp_avg_sqs[s]: the moments in the
    parameter's dtype, written, and read unless first[s].  step: the count after the increment.
    The hyperparameters, `betas` (a (beta1, beta2) pair), `step`, `decoupled` and `first` are
    scalars or per-tensor lists.  gclip / write_clipped / sr: ParamAdamPlan.run's.  Returns the
    plan (pass it back in to reuse its tables)."""
    plan = _adam_tables(params, grads, exp_avgs, exp_avg_sqs, lr, betas, eps, weight_decay, step, decoupled, first,
                        plan, False)
    plan.run(flat, write, gclip, write_clipped, sr)
    return plan


def params_adam_master(params, grads, exp_avgs, exp_avg_sqs, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                       step=1, decoupled=False, first=False, master=None, write=True, gclip=None, write_clipped=False,
                       plan=None):
    """The Adam / AdamW update on fp32 master weights (include/choco_codec.h,
    choco_params_adam_master): params_adam's arguments, except that the update runs in place on
    `master` -- the persistent flat fp32 copy of `params`, laid out back to back -- and the
    moments are fp32 tensors whatever their parameter's dtype.  grads[s] None: the tensor is
    passed over.  write: the parameters receive the new master values narrowed to their dtype.
    Returns the plan (pass it back in to reuse its tables)."""
    if master is None:
        raise RuntimeError("params_adam_master needs the master buffer")
    plan = _adam_tables(params, grads, exp_avgs, exp_avg_sqs, lr, betas, eps, weight_decay, step, decoupled, first,
                        plan, True)
    plan.run_master(master, write, gclip, write_clipped)
    return plan


def params_sqnorm_launches(nseg):
    """Launches one params_sqnorm of `nseg` tensors takes."""
    return int(lib().choco_params_sqnorm_launches(int(nseg)))


def params_sqnorm(params, grads, weight_decay=0.0, plan=None):
    """Per-tensor L2 norms of d = g, or fma(wd, p, g) where weight_decay != 0 (scalar or
    per-tensor list): DGC._clip_gradient's grad.norm(p=2) (dgc.py:254-256) for a whole list in
    one batched launch per chunk plus a finish launch, fp64 accumulation in a fixed order.
    grads[s] None: norm 0.  Returns the plan's fp32 norms tensor (pass `plan` back in to reuse
    its tables and workspace; the tensor is overwritten by the plan's next sqnorm)."""
    params = list(params)
    nseg = len(params)
    if plan is None:
        plan = ParamSgdPlan(params)
    elif not plan.holds(params):
        raise RuntimeError("the plan was built for another parameter list")
    grads, wds = _per_tensor(grads, nseg, "grads"), _per_tensor(weight_decay, nseg, "weight_decay")
    for i, (p, g, wd) in enumerate(zip(params, grads, wds)):
        if g is not None and not plan.fits(i, g):
            raise RuntimeError(f"grad {i} must match its parameter's dtype, device and size, and be contiguous")
        plan.param_ptrs[i] = p.data_ptr()
        plan.grad_ptrs[i] = g.data_ptr() if g is not None else None
        plan.flags[i] = SGD_F_NOGRAD if g is None else 0
        plan.weight_decay[i] = wd
        plan.seen[i] = None
    return plan.sqnorm()


def params_mask_launches(nseg):
    """Launches one params_mask of `nseg` tensors takes."""
    return int(lib().choco_params_mask_launches(int(nseg)))


def params_mask(bufs, values, indices, k_per_seg, memory=None, lens=None, dtypes=None):
    """DGC's momentum-factor masking (dgc.py:178-182) and the clear of the error-feedback memory
    at the selected positions (:174-176), one batched launch per chunk of tensors: for slot j of
    tensor s, bufs[s].view(-1)[indices[j] - off_s] *= 0 and memory[indices[j]] = v + (-v), v =
    values[j].  values / indices: a segmented selection (global ascending int32 indices) with
    k_per_seg[s] slots per tensor.  bufs[s] may be None (no buffer to mask); then `lens` (and,
    for 16-bit layouts, `dtypes`) give the layout, which otherwise comes from the buffers."""
    bufs = list(bufs)
    nseg = len(bufs)
    _require(values, torch.float32, "values")
    _require(indices, torch.int32, "indices")
    dev = values.device
    if len(k_per_seg) != nseg or indices.numel() != values.numel():
        raise RuntimeError("k_per_seg needs one entry per tensor, indices one per value")
    if lens is None:
        if any(b is None for b in bufs):
            raise RuntimeError("params_mask needs `lens` when a buffer is None")
        lens = [b.numel() for b in bufs]
    if len(lens) != nseg:
        raise RuntimeError(f"lens: {len(lens)} values for {nseg} tensors")
    ptrs, c_lens, dts, ks = ((ctypes.c_void_p * nseg)(), (ctypes.c_int64 * nseg)(), (ctypes.c_int32 * nseg)(),
                             (ctypes.c_int64 * nseg)())
    for i, b in enumerate(bufs):
        if b is not None:
            _require(b, None, f"buf {i}")
            if b.device != dev or b.numel() != lens[i] or b.dtype not in PARAM_DTYPES:
                raise RuntimeError(f"buf {i} must hold {lens[i]} fp32 / bf16 / fp16 elements on {dev}")
            if dtypes is not None and dtypes[i] != b.dtype:
                raise RuntimeError(f"buf {i} is {b.dtype}, dtypes says {dtypes[i]}")
            ptrs[i], dts[i] = b.data_ptr(), PARAM_DTYPES[b.dtype]
        else:
            ptrs[i], dts[i] = None, PARAM_DTYPES[dtypes[i]] if dtypes is not None else 0
        c_lens[i], ks[i] = int(lens[i]), int(k_per_seg[i])
    n = sum(int(m) for m in lens)
    if memory is not None:
        _require(memory, torch.float32, "memory")
        if memory.device != dev or memory.numel() != n:
            raise RuntimeError(f"memory must hold {n} elements on {dev}")
    _lib.check(lib().choco_params_mask(ptrs, c_lens, dts, ks, nseg, _ptr(values), _ptr(indices), values.numel(),
                                       _ptr(memory), n, _stream(dev)), "choco_params_mask")


# ----------------------------------------------------------------------------- profiling
def profile_enable(on=True):
    lib().choco_profile_enable(1 if on else 0)


def profile_filter(names=None):
    """Time only the launches named in `names` (a name or a list; None = all)."""
    if isinstance(names, (list, tuple)):
        names = ",".join(names)
    lib().choco_profile_filter(names.encode() if names else None)


def profile_read(name):
    total = ctypes.c_double(0.0)
    cnt = ctypes.c_int64(0)
    lib().choco_profile_read(name.encode(), ctypes.byref(total), ctypes.byref(cnt))
    return total.value, cnt.value


def profile_reset():
    lib().choco_profile_reset()


def launch_count(name):
    """Launches of kernel `name` since the library was loaded (counted with profiling off)."""
    return int(lib().choco_launch_count(name.encode()))


def topk_workspace_word(off, dev=None, plan=None):
    """Diagnostic: the uint32 at byte `off` of this stream's flat top-k workspace (or of
    `plan`'s segmented one); include/choco_codec.h CHOCO_TOPK_*_OFFSET.  Synchronises."""
    dev = torch.device(dev) if dev is not None else torch.device("cuda", torch.cuda.current_device())
    if plan is not None:
        ws = plan.workspace(dev)
    else:
        with _ws_lock:
            ws = _ws_cache.get((dev.index, torch.cuda.current_stream(dev).cuda_stream, "topk"))
        if ws is None:
            return 0
    torch.cuda.current_stream(dev).synchronize()
    return int(ws[off:off + 4].view(torch.int32).item())


SEG_WIN_WORDS = ("lo", "sh", "valid", "pad", "t_prev", "d_prev", "cand", "trust")
SEG_HOST_WORDS = ("calls", "last_flag", "cold_left", "backoff", "clean", "last_checks", "last_misses", "flag")


def seg_diag_layout(plan):
    """Diagnostic: byte offsets (win, info) of the per-segment windows and info rows in
    `plan`'s workspace (include/choco_codec.h CHOCO_SEG_*).  Host only."""
    win, info = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib().choco_topk_segmented_diag_layout(plan.plan_host, plan.nseg, ctypes.byref(win),
                                                      ctypes.byref(info)), "choco_topk_segmented_diag_layout")
    return int(win.value), int(info.value)


def _seg_rows(plan, off, stride, dev):
    dev = torch.device(dev) if dev is not None else torch.device("cuda", torch.cuda.current_device())
    ws = plan.workspace(dev)
    torch.cuda.current_stream(dev).synchronize()
    rows = ws[off:off + stride * plan.nseg].cpu().numpy().view("<u4")
    return rows.reshape(plan.nseg, stride // 4).copy()


def seg_windows(plan, dev=None):
    """Diagnostic: the (nseg, 8) uint32 array of `plan`'s warm windows, columns SEG_WIN_WORDS
    (rows of single-tile and flat-pipeline segments stay zero).  Synchronises the stream."""
    return _seg_rows(plan, seg_diag_layout(plan)[0], _lib.SEG_WIN_STRIDE, dev)


def seg_info(plan, dev=None):
    """Diagnostic: the (nseg, 8) uint32 array of `plan`'s info rows (after a warm call: word
    _lib.SEG_INFO_LO / SEG_INFO_SH the window used, SEG_INFO_MODE how it went).  Synchronises."""
    return _seg_rows(plan, seg_diag_layout(plan)[1], _lib.SEG_INFO_STRIDE, dev)


def seg_shadow(plan, dev=None):
    """Diagnostic: the cold calls' window-check counter of `plan`'s workspace as (misses,
    checks) (CHOCO_SEG_SHADOW_OFFSET).  Synchronises."""
    lo = topk_workspace_word(_lib.SEG_SHADOW_OFFSET, dev=dev, plan=plan) & 0xFFFFFFFF
    hi = topk_workspace_word(_lib.SEG_SHADOW_OFFSET + 4, dev=dev, plan=plan) & 0xFFFFFFFF
    return hi, lo


def seg_host_state(plan, dev=None):
    """Diagnostic: the host's warm / cold bookkeeping of `plan`'s workspace on this stream
    as a dict over SEG_HOST_WORDS (all zeros before the first call).  Host memory only: no
    synchronisation, no copy."""
    dev = torch.device(dev) if dev is not None else torch.device("cuda", torch.cuda.current_device())
    out = (ctypes.c_uint64 * 8)()
    _lib.check(lib().choco_topk_segmented_host_state(_ptr(plan.workspace(dev)), plan.plan_host, plan.nseg, out),
               "choco_topk_segmented_host_state")
    return dict(zip(SEG_HOST_WORDS, (int(v) for v in out)))


def is_pow2_minus1(s):
    return s >= 1 and (s + 1) & s == 0 and int(math.log2(s + 1)) <= 16
