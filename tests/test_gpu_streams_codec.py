"""Every launching wrapper of codec.py on a delayed side stream (tests/_streams.py), against the
oracles its own test uses: a launch, memset or copy inside the library that is handed another
stream than the caller's reads poison or writes too late, and the numbers differ.

The harness is tested first, on deliberate mis-streamings of a plain copy (no project code).  The
cases follow, one per wrapper and variant, at the smallest size that takes every launch of the
multi-launch paths (70 001 elements: top-k's sample + stream + select, a third partial sign column
block; 40 000: top-k's one-workgroup path; [33, 31, 70 001]: rows split over segments).  The
harness's warm-ups leave top-k warm, and a warm call skips the sample kernel (segmented: the two
histogram passes), so every top-k case at 70 001 also runs cold: each call on a workspace the
library has never seen (class Fresh), with the launch counter showing that the delayed call did
take the skipped launch.  Random-k keeps no state between calls: its launches are the same every
call.  One host
test keeps the table complete: every public callable of codec.py whose source passes `_stream(`
is in a case's `covers` or in EXEMPT.

Bit for bit, but for the device norms of sign / QSGD (rtol 1e-6, their own tests' bound)."""
import collections
import inspect
import re
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _streams as ST
from conftest import same_bits
from oracle import choco_oracle as O

DEV = "cuda"
F32 = np.float32
GAMMA = 0.9
gpu = pytest.mark.gpu

FLAT = [70_001]
SEG3 = [33, 31, 70_001]
TOPK_LENS = [3, 70_001, 5, 300]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def host(obj):
    if torch.is_tensor(obj):
        return obj.cpu().numpy() if obj.dtype != torch.bfloat16 else obj.float().cpu().numpy()
    if isinstance(obj, dict):
        return {k: host(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [host(v) for v in obj]
    return obj


def randn(n, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(F32)


def state(n, seed):
    """x, x_hat, memory as a CHOCO step meets them (test_gpu_gossip_fused._inputs, on the host)."""
    x = randn(n, seed)
    hat = (x + randn(n, seed + 1, 0.1)).astype(F32)
    mem = (hat + randn(n, seed + 2, 0.05)).astype(F32)
    return x, hat, mem


def seg_table(lens):
    return dev(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)) if len(lens) > 1 else None


def auto_poison(name, a):
    """Valid but wrong: other finite normals.  Only floats: indices, packed words and norms get their
    poison from the case."""
    assert a.dtype == F32, f"{name}: give the poison of a {a.dtype} input"
    return randn(a.size, zlib.crc32(name.encode()) + 17).reshape(a.shape)


def go(family, case, call, true, poison=None, outs=None, **kw):
    """One call under the harness.  true / poison: {name: numpy array}; outs: {name: (numel, torch
    dtype)} pre-allocated and SENTINEL-filled; call(W) takes the working tensors (inputs and outs) as
    W.name.  Returns (what the call returned, the working tensors, the outs) as numpy, read on the
    side stream right behind the call."""
    poison = dict(poison or {})
    for k, a in true.items():
        if k not in poison:
            poison[k] = auto_poison(k, a)
        assert poison[k].shape == a.shape and poison[k].dtype == a.dtype, k
    up = lambda a: a.to(DEV) if torch.is_tensor(a) else dev(a)  # noqa: E731  (a CPU tensor: a bf16 storage)
    t_true = {k: up(a) for k, a in true.items()}
    t_poison = {k: up(a) for k, a in poison.items()}
    work = {k: torch.empty_like(t) for k, t in t_true.items()}
    out_t = {k: torch.empty(m, dtype=dt, device=DEV) for k, (m, dt) in (outs or {}).items()}
    W = SimpleNamespace(**work, **out_t)
    ret, w, o = ST.run(lambda: call(W), work, t_true, t_poison, outs=list(out_t.values()), family=family, case=case,
                       **kw)
    return host(ret), SimpleNamespace(**host(w)), SimpleNamespace(**dict(zip(out_t, host(o))))


# ------------------------------------------------------------------------------ the harness itself
def _copy_case(stream_of_copy, **kw):
    """y.copy_(x) queued on `stream_of_copy(S)` inside the side-stream block; returns (y read on S, x)."""
    x = randn(4096, 1)

    def call(W):
        with torch.cuda.stream(stream_of_copy(torch.cuda.current_stream())):
            W.y.copy_(W.x)

    _, _, o = go("harness", "copy", call, {"x": x}, outs={"y": (4096, torch.float32)}, **kw)
    return o.y, x


@gpu
def test_harness_flags_a_read_on_the_null_stream():
    """Read early: the null-stream copy runs during S's delay and copies the poison."""
    y, x = _copy_case(lambda s: torch.cuda.default_stream(), write_late=False)
    assert not same_bits(y, x)
    assert np.all(np.isfinite(y)) and not np.any(y == ST.SENTINEL), "it read the poison, a valid input"


@gpu
def test_harness_flags_a_write_on_the_null_stream():
    """Write late: the null-stream copy is held back and S's read of y sees the sentinel."""
    y, x = _copy_case(lambda s: torch.cuda.default_stream(), read_early=False)
    assert np.all(y == ST.SENTINEL)


@gpu
def test_harness_flags_the_null_stream_with_both_delays():
    y, x = _copy_case(lambda s: torch.cuda.default_stream())
    assert not same_bits(y, x)


@gpu
@pytest.mark.parametrize("kw", [dict(write_late=False), dict(read_early=False), dict()],
                         ids=["read_early", "write_late", "both"])
def test_harness_passes_the_copy_on_the_side_stream(kw):
    y, x = _copy_case(lambda s: s, **kw)
    assert same_bits(y, x)
    ST.print_report("harness")


# ------------------------------------------------------------------------------ the case table
Case = collections.namedtuple("Case", "family covers fn")
CASES = {}


def case(family, name, covers):
    def reg(fn):
        assert name not in CASES
        CASES[name] = Case(family, tuple(covers), fn)
        return fn
    return reg


class Fresh:
    """Cold calls: every call of a case -- the warm-ups and the delayed one -- gets a zero-filled workspace
    the library has never seen, as codec.workspace / SegmentPlan.workspace make them on a stream's first
    call.  A warm workspace skips what only a first call launches (flat top-k: the sample kernel; the
    hash mode of random-k: the hipMemsetAsync pair; segmented: the S1 + S2 histogram passes), and the
    harness's warm-ups would leave only warm calls behind the delay.  The workspaces are allocated, zeroed
    and synchronised beforehand on the side stream; `install(buf)` puts one where the wrapper looks."""

    def __init__(self, nbytes, install, count=3):
        from chocosgd_amd import codec
        self.install, self.used = install, 0
        with torch.cuda.stream(ST.side_stream()):
            self.bufs = [codec._new_workspace(torch.device(DEV, 0), max(int(nbytes), 256)) for _ in range(count)]
        torch.cuda.synchronize()

    def next(self):
        self.install(self.bufs[self.used])
        self.used += 1

    def close(self):
        """The library's and the shim's host-side state of these addresses goes with them."""
        from chocosgd_amd import codec
        torch.cuda.synchronize()
        for b in self.bufs:
            codec._status.pop(b.data_ptr(), None)
            codec.lib().choco_topk_workspace_reset(codec._ptr(b), b.numel())


def flat_workspace_slot(kind):
    """(install, restore) of the side stream's cached `kind` workspace of codec.workspace."""
    from chocosgd_amd import codec
    key = (0, ST.side_stream().cuda_stream, kind)
    old = codec._ws_cache.get(key)

    def restore():
        if old is None:
            codec._ws_cache.pop(key, None)
        else:
            codec._ws_cache[key] = old
    return (lambda buf: codec._ws_cache.__setitem__(key, buf)), restore


# ---- top-k, flat
def _topk_flat(n, variant, cold=False):
    from chocosgd_amd import codec
    k = O.topk_k(n, 0.99)
    fresh, sampled = None, []
    if cold:
        install, restore = flat_workspace_slot("topk")
        fresh = Fresh(codec.lib().choco_topk_workspace_size(n), install)
    x, hat, mem = state(n, n)
    outs = {"vals": (k, torch.float32), "idx": (k, torch.int32)}
    w = 1.0 / 3

    def call(W):
        if cold:
            fresh.next()
            c0 = codec.launch_count("topk_bounds")
        if variant == "plain":
            if not cold:
                codec.topk(W.x, k, out=(W.vals, W.idx))
            ret = codec.topk(W.x, k, out=(W.vals, W.idx))  # (warm: the second call, on this stream's workspace)
        elif variant == "xhat":
            if not cold:
                codec.topk(W.x, k, xhat=W.hat, out=(W.vals, W.idx))
            ret = codec.topk(W.x, k, xhat=W.hat, out=(W.vals, W.idx))
        elif variant == "gossip":
            ret = codec.topk(W.x, k, xhat=W.hat, out=(W.vals, W.idx), gossip=(W.mem, GAMMA))
        else:
            ret = codec.topk(W.x, k, xhat=W.hat, out=(W.vals, W.idx), fold=(W.hat, W.mem, w))
        if cold:
            sampled.append(codec.launch_count("topk_bounds") - c0)
        return ret

    try:
        _, W, o = go("topk", f"topk-{n}-{variant}" + ("-cold" if cold else ""), call,
                     {"x": x, "hat": hat, "mem": mem}, outs=outs, warm=2)
    finally:
        if cold:
            restore()
            fresh.close()
    if cold:
        assert sampled == [1, 1, 1], f"the sample kernel's launches per call: {sampled}"
    xa = O.gossip_step(x, mem, hat, GAMMA) if variant == "gossip" else x
    d = xa if variant == "plain" else (xa - hat).astype(F32)
    ov, oi = O.topk(d, k)
    assert np.array_equal(o.idx.astype(np.int64), oi) and same_bits(o.vals, ov)
    assert same_bits(W.x, xa)
    h, m = hat.copy(), mem.copy()
    if variant == "fold":
        O.sparse_accumulate(h, m, ov, oi, w)
    assert same_bits(W.hat, h) and same_bits(W.mem, m)


for _n in (70_001, 40_000):
    for _v in ("plain", "xhat", "gossip", "fold"):
        case("topk", f"topk-{_n}-{_v}", ["topk"])(lambda n=_n, v=_v: _topk_flat(n, v))
for _v in ("plain", "xhat", "gossip", "fold"):  # sample + stream + select behind the delay
    case("topk", f"topk-70001-{_v}-cold", ["topk"])(lambda v=_v: _topk_flat(70_001, v, cold=True))


# ---- top-k / random-k, segmented; random-k flat; gather
def _segmented(kind, gossip, cold=False):
    """cold (top-k): every call is the first on its plan workspace, so the delayed one runs the histogram
    passes S1 + S2 in front of the select; otherwise it is warm from the warm-ups (collect, bin, emit)."""
    from chocosgd_amd import codec
    lens, n = TOPK_LENS, sum(TOPK_LENS)
    x, hat, mem = state(n, 7)
    plan = codec.SegmentPlan(lens, 0.99, torch.device(DEV, 0))
    outs = {"vals": (plan.k_total, torch.float32), "idx": (plan.k_total, torch.int32)}
    g = (lambda W: (W.mem, GAMMA)) if gossip else (lambda W: None)
    fresh, hist = None, []
    if cold:
        key = (0, ST.side_stream().cuda_stream)
        fresh = Fresh(plan.ws_bytes, lambda buf: plan._ws.__setitem__(key, buf))

    def call(W):
        if cold:
            fresh.next()
        c0 = codec.launch_count("topk_seg_hist")
        if kind == "topk":
            ret = codec.topk_segmented(W.x, plan, xhat=W.hat, out=(W.vals, W.idx), gossip=g(W))
        else:
            ret = codec.randk_segmented(W.x, plan, 1234, xhat=W.hat, out=(W.vals, W.idx), gossip=g(W))
        hist.append(codec.launch_count("topk_seg_hist") - c0)
        return ret

    try:
        _, W, o = go("segmented", f"{kind}_segmented-{'gossip' if gossip else 'plain'}" + ("-cold" if cold else ""),
                     call, {"x": x, "hat": hat, "mem": mem}, outs=outs, warm=2)
    finally:
        if cold:
            plan._ws.clear()
            fresh.close()
    if cold:
        assert hist == [1, 1, 1], f"the histogram pass's launches per call: {hist}"
    xa = O.gossip_step(x, mem, hat, GAMMA) if gossip else x
    d = (xa - hat).astype(F32)
    ov, oi = O.topk_segmented(d, lens, 0.99)[:2] if kind == "topk" else O.randk_segmented(d, lens, 0.99, 1234)
    assert np.array_equal(o.idx.astype(np.int64), oi) and same_bits(o.vals, ov)
    assert same_bits(W.x, xa) and same_bits(W.hat, hat) and same_bits(W.mem, mem)


for _k in ("topk", "randk"):
    for _g in (False, True):
        case("segmented", f"{_k}_segmented-{'gossip' if _g else 'plain'}", [f"{_k}_segmented"])(
            lambda k=_k, g=_g: _segmented(k, g))
for _g in (False, True):
    case("segmented", f"topk_segmented-{'gossip' if _g else 'plain'}-cold", ["topk_segmented"])(
        lambda g=_g: _segmented("topk", g, cold=True))


@case("segmented", "randk-flat", ["randk"])
def _randk_flat():
    from chocosgd_amd import codec
    n = 70_001
    k = O.topk_k(n, 0.99)
    x, hat, _ = state(n, 21)
    _, W, o = go("segmented", "randk-flat",
                 lambda W: codec.randk(W.x, k, 99, is_biased=False, xhat=W.hat, offset=3, out=(W.vals, W.idx)),
                 {"x": x, "hat": hat}, outs={"vals": (k, torch.float32), "idx": (k, torch.int32)})
    oi = O.randk_indices(n, k, 99, 3)
    assert np.array_equal(o.idx.astype(np.int64), oi)
    assert same_bits(o.vals, O.gather((x - hat).astype(F32), oi, n, k, is_biased=False))


@case("segmented", "gather", ["gather"])
def _gather():
    from chocosgd_amd import codec
    n, k = 70_001, 5_000
    x, hat, _ = state(n, 22)
    idx = np.sort(np.random.default_rng(5).choice(n, size=k, replace=False)).astype(np.int64)
    ret, _, _ = go("segmented", "gather", lambda W: codec.gather(W.x, W.idx, 1.0, xhat=W.hat),
                   {"x": x, "hat": hat, "idx": idx}, poison={"idx": np.arange(k, dtype=np.int64)})
    assert same_bits(ret, O.gather((x - hat).astype(F32), idx))


# ---- sparse receivers
def _sparse_msg(n, k, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(k).astype(F32), np.sort(rng.choice(n, size=k, replace=False)).astype(np.int32))


@case("sparse", "sparse_accumulate+guard", ["sparse_accumulate", "IndexGuard.arm", "IndexGuard.check"])
def _sparse_accumulate():
    """One index past the end: skipped and counted.  The guard's copy, armed on the side stream behind
    the launch, must bring back that count -- a copy on another stream brings the 0 of before."""
    from chocosgd_amd import codec
    n, k = 100_000, 5_000
    vals, idx = _sparse_msg(n, k, 31)
    idx[-1] = n + 5
    hat, mem = randn(n, 32), randn(n, 33)
    guard = codec.IndexGuard(torch.device(DEV, 0))
    true_word = np.zeros(1, np.int32)

    def call(W):
        guard.word = W.word  # (fresh per run: the count is cumulative)
        codec.sparse_accumulate(W.vals, W.idx, W.mem, 0.25, xhat_self=W.hat, guard=guard)
        guard.arm()

    _, W, _ = go("sparse", "sparse_accumulate+guard", call,
                 {"vals": vals, "idx": idx, "hat": hat, "mem": mem, "word": true_word},
                 poison={"idx": np.arange(k, dtype=np.int32), "word": true_word})
    h, m = hat.copy(), mem.copy()
    O.sparse_accumulate(h, m, vals[:-1], idx[:-1], 0.25)
    assert same_bits(W.hat, h) and same_bits(W.mem, m)
    with pytest.raises(RuntimeError, match="1 received indices out of range"):
        guard.check(wait=True)


def _sparse_multi(nmsg):
    from chocosgd_amd import codec
    import test_gpu_sparse_multi as SM
    n, slot = 100_000, nmsg // 2
    msgs = SM._messages(n, [5_000 - 100 * m for m in range(nmsg)], seed=nmsg)
    weights = [0.3] + [1.0 / nmsg] * (nmsg - 1)
    hat, mem = randn(n, 41), randn(n, 42)
    true = {"hat": hat, "mem": mem}
    poison = {}
    for m, (v, i) in enumerate(msgs):
        true[f"v{m}"], true[f"i{m}"] = v, i.astype(np.int32)
        poison[f"i{m}"] = np.arange(i.size, dtype=np.int32)

    def call(W):
        dm = [(getattr(W, f"v{m}"), getattr(W, f"i{m}")) for m in range(nmsg)]
        codec.sparse_accumulate_multi(dm, weights, W.mem, self_slot=slot, xhat_self=W.hat)

    _, W, _ = go("sparse", f"sparse_accumulate_multi-{nmsg}", call, true, poison=poison)
    h, m_ = hat.copy(), mem.copy()
    for s, ((v, i), w) in enumerate(zip(msgs, weights)):
        O.sparse_accumulate(h if s == slot else None, m_, v, i, w)
    assert same_bits(W.hat, h) and same_bits(W.mem, m_)


for _m in (3, 10):
    case("sparse", f"sparse_accumulate_multi-{_m}", ["sparse_accumulate_multi"])(lambda m=_m: _sparse_multi(m))


@case("sparse", "sparse_extrapolate", ["sparse_extrapolate"])
def _sparse_extrapolate():
    from chocosgd_amd import codec
    n, k = 100_000, 5_000
    vals, idx = _sparse_msg(n, k, 51)
    t0 = randn(n, 52)
    a, b = O.ecd_coeffs(3)
    _, W, _ = go("sparse", "sparse_extrapolate",
                 lambda W: codec.sparse_extrapolate(W.vals, W.idx, W.t, float(a), float(b)),
                 {"vals": vals, "idx": idx, "t": t0}, poison={"idx": np.arange(k, dtype=np.int32)})
    want = t0.copy()
    want[idx] = O.fma32(b, vals, (t0[idx] * a).astype(F32))
    assert same_bits(W.t, want)


# ---- sign
def _sign_compress(lens, gossip, ranges):
    from chocosgd_amd import codec
    n, nseg = sum(lens), len(lens)
    x, hat, mem = state(n, 9 + nseg)
    so = seg_table(lens)
    words = O.sign_words(n)
    chunks = codec.sign_chunks(n, 2)
    assert len(chunks) == 2

    def call(W):
        g = (W.mem, GAMMA) if gossip else None
        if not ranges:
            return codec.sign_compress(W.x, xhat=W.hat, seg_off=so, nseg=nseg, gossip=g, out=(W.packed, W.norms))
        for i, (w0, w1) in enumerate(chunks):
            codec.sign_compress_range(W.x, w0, w1, i == 1, xhat=W.hat, seg_off=so, nseg=nseg, gossip=g,
                                      out=(W.packed, W.norms))

    name = f"sign_compress{'_range' if ranges else ''}-{nseg}seg-{'gossip' if gossip else 'plain'}"
    _, W, o = go("sign", name, call, {"x": x, "hat": hat, "mem": mem},
                 outs={"packed": (words, torch.int32), "norms": (nseg, torch.float32)})
    xa = O.gossip_step(x, mem, hat, GAMMA) if gossip else x
    d = (xa - hat).astype(F32)
    assert same_bits(W.x, xa) and same_bits(W.hat, hat) and same_bits(W.mem, mem)
    assert np.array_equal(o.packed, O.sign_pack(d))
    assert np.allclose(o.norms, O.l1_norms(d, lens), rtol=1e-6, atol=0)


for _l in (FLAT, SEG3):
    for _g in (False, True):
        case("sign", f"sign_compress-{len(_l)}seg-{'gossip' if _g else 'plain'}", ["sign_compress"])(
            lambda l=_l, g=_g: _sign_compress(l, g, False))
for _g in (False, True):
    case("sign", f"sign_compress_range-3seg-{'gossip' if _g else 'plain'}", ["sign_compress_range"])(
        lambda g=_g: _sign_compress(SEG3, g, True))


def _sign_msgs(n, lens, nmsg, seed):
    """[(words, norms)] made on the host (test_gpu_receivers.scase's recipe) and their poison: other
    well-formed words, norms of 1."""
    rng = np.random.default_rng([seed, n, nmsg])
    true, poison = {}, {}
    for m in range(nmsg):
        true[f"p{m}"] = O.sign_pack(rng.standard_normal(n).astype(F32))
        true[f"n{m}"] = (rng.uniform(0.2, 2.0, size=len(lens)) * np.array(lens)).astype(F32)
        poison[f"p{m}"] = O.sign_pack(rng.standard_normal(n).astype(F32))
        poison[f"n{m}"] = np.ones(len(lens), F32)
    return true, poison


def _msgs_of(W, nmsg):
    return [(getattr(W, f"p{m}"), getattr(W, f"n{m}")) for m in range(nmsg)]


def _weights(nmsg):
    return [1 / 3, -0.5, 1.0, 0.125, 0.3, 0.7, -1.0, 0.2, 0.45, -0.15][:nmsg]


@case("sign", "sign_unpack", ["sign_unpack"])
def _sign_unpack():
    from chocosgd_amd import codec
    n = 70_001
    true, poison = _sign_msgs(n, FLAT, 1, 1)
    ret, _, _ = go("sign", "sign_unpack", lambda W: codec.sign_unpack(W.p0, n), {"p0": true["p0"]},
                   poison={"p0": poison["p0"]})
    assert same_bits(ret, O.sign_unpack(true["p0"], n))


def _sign_accumulate(nmsg):
    from chocosgd_amd import codec
    lens, n, slot = SEG3, sum(SEG3), 1
    true, poison = _sign_msgs(n, lens, nmsg, 2)
    hat, mem = randn(n, 61), randn(n, 62)
    so, w = seg_table(lens), _weights(nmsg)
    _, W, _ = go("sign", f"sign_accumulate-{nmsg}",
                 lambda W: codec.sign_accumulate(_msgs_of(W, nmsg), w, slot, n, W.mem, xhat_self=W.hat, seg_off=so,
                                                 nseg=len(lens)),
                 dict(true, hat=hat, mem=mem), poison=poison)
    h, m_ = hat.copy(), mem.copy()
    O.sign_accumulate(h, m_, [(true[f"p{m}"], true[f"n{m}"]) for m in range(nmsg)], w, slot, lens)
    assert same_bits(W.hat, h) and same_bits(W.mem, m_)


for _m in (3, 10):
    case("sign", f"sign_accumulate-{_m}", ["sign_accumulate"])(lambda m=_m: _sign_accumulate(m))


def _sign_axpy(two_roundings):
    from chocosgd_amd import codec
    lens, n, nmsg = SEG3, sum(SEG3), 3
    true, poison = _sign_msgs(n, lens, nmsg, 3)
    t0 = randn(n, 63)
    so, w = seg_table(lens), _weights(nmsg)
    _, W, _ = go("sign", f"sign_axpy-{'two' if two_roundings else 'fma'}",
                 lambda W: codec.sign_axpy(_msgs_of(W, nmsg), w, n, W.t, seg_off=so, nseg=len(lens),
                                           two_roundings=two_roundings),
                 dict(true, t=t0), poison=poison)
    want = t0.copy()
    for m in range(nmsg):
        O.sign_axpy(want, true[f"p{m}"], true[f"n{m}"], lens, w[m], two_roundings)
    assert same_bits(W.t, want)


for _t in (False, True):
    case("sign", f"sign_axpy-{'two' if _t else 'fma'}", ["sign_axpy"])(lambda t=_t: _sign_axpy(t))


@case("sign", "sign_extrapolate", ["sign_extrapolate"])
def _sign_extrapolate():
    from chocosgd_amd import codec
    lens, n = SEG3, sum(SEG3)
    true, poison = _sign_msgs(n, lens, 1, 4)
    t0 = randn(n, 64)
    so = seg_table(lens)
    a, b = O.ecd_coeffs(3)
    _, W, _ = go("sign", "sign_extrapolate",
                 lambda W: codec.sign_extrapolate(W.p0, W.n0, n, W.t, float(a), float(b), seg_off=so, nseg=len(lens)),
                 dict(true, t=t0), poison=poison)
    assert same_bits(W.t, O.ecd_sign_extrapolate(t0, true["p0"], true["n0"], lens, 3))


def _local_norms(lens, seed):
    return (np.random.default_rng(seed).uniform(0.2, 2.0, size=len(lens)) * np.array(lens)).astype(F32)


@case("sign", "sign_local_decode", ["sign_local_decode"])
def _sign_local_decode():
    from chocosgd_amd import codec
    lens, n = SEG3, sum(SEG3)
    x, norms, so = randn(n, 65), _local_norms(SEG3, 66), seg_table(SEG3)
    ret, _, _ = go("sign", "sign_local_decode",
                   lambda W: codec.sign_local_decode(W.x, W.norms, seg_off=so, nseg=len(lens)),
                   {"x": x, "norms": norms}, poison={"norms": np.ones(len(lens), F32)})
    assert same_bits(ret, O.sign_local(x, norms, lens))


@case("sign", "sign_local_residual", ["sign_local_residual"])
def _sign_local_residual():
    from chocosgd_amd import codec
    import _ef_oracle as EO
    lens, n = SEG3, sum(SEG3)
    x, norms, so = randn(n, 67), _local_norms(SEG3, 68), seg_table(SEG3)
    _, W, o = go("sign", "sign_local_residual",
                 lambda W: codec.sign_local_residual(W.x, W.norms, seg_off=so, nseg=len(lens), local_out=W.local,
                                                     resid_out=W.resid),
                 {"x": x, "norms": norms}, poison={"norms": np.ones(len(lens), F32)},
                 outs={"local": (n, torch.float32), "resid": (n, torch.float32)})
    want_r, want_u = EO.residual(x, norms, lens)
    assert same_bits(o.resid, want_r) and same_bits(o.local, want_u) and same_bits(W.x, x)


def _sign_recv(nmsg):
    """More than eight messages: the leading two go through sign_accumulate, the rest with the
    consensus step and the pack through the fused kernel."""
    from chocosgd_amd import codec
    lens, n, slot = SEG3, sum(SEG3), 1
    true, poison = _sign_msgs(n, lens, nmsg, 5)
    x, hat, mem = state(n, 69)
    so, w = seg_table(lens), _weights(nmsg)
    _, W, o = go("sign", f"sign_recv_gossip_compress-{nmsg}",
                 lambda W: codec.sign_recv_gossip_compress(_msgs_of(W, nmsg), w, slot, W.x, W.mem, W.hat, GAMMA,
                                                           seg_off=so, nseg=len(lens), out=(W.packed, W.norms)),
                 dict(true, x=x, hat=hat, mem=mem), poison=poison,
                 outs={"packed": (O.sign_words(n), torch.int32), "norms": (len(lens), torch.float32)})
    h, m_ = hat.copy(), mem.copy()
    O.sign_accumulate(h, m_, [(true[f"p{m}"], true[f"n{m}"]) for m in range(nmsg)], w, slot, lens)
    xa = O.gossip_step(x, m_, h, GAMMA)
    d = (xa - h).astype(F32)
    assert same_bits(W.hat, h) and same_bits(W.mem, m_) and same_bits(W.x, xa)
    assert np.array_equal(o.packed, O.sign_pack(d))
    assert np.allclose(o.norms, O.l1_norms(d, lens), rtol=1e-6, atol=0)


for _m in (3, 10):
    case("sign", f"sign_recv_gossip_compress-{_m}", ["sign_recv_gossip_compress"])(lambda m=_m: _sign_recv(m))


# ---- QSGD, q = 4
Q, S_LEVELS = 4, 15


def _bounds(lens):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return list(zip(off[:-1].tolist(), off[1:].tolist()))


def _qsgd_levels(d, lens, norms, seed, offset):
    u = O.qsgd_uniforms(d.size, seed, offset)
    return np.concatenate([O.qsgd_levels(d[a:b], S_LEVELS, u[a:b], norms[i]) for i, (a, b) in enumerate(_bounds(lens))])


def _qsgd_compress(lens, gossip):
    """The norm pass, then the quantize pass; the wire against the oracle at the device's norms (as
    test_gossip_qsgd does) and those within rtol 1e-6 of the fp64 norms."""
    from chocosgd_amd import codec
    n, nseg = sum(lens), len(lens)
    x, hat, mem = state(n, 70 + nseg)
    so = seg_table(lens)

    def call(W):
        return codec.qsgd_compress(W.x, Q, xhat=W.hat, seg_off=so, nseg=nseg, seed=77, offset=5,
                                   gossip=(W.mem, GAMMA) if gossip else None, out=(W.packed, W.norms))

    _, W, o = go("qsgd", f"qsgd_compress-{nseg}seg-{'gossip' if gossip else 'plain'}", call,
                 {"x": x, "hat": hat, "mem": mem},
                 outs={"packed": (codec.qsgd_packed_bytes(n, Q), torch.uint8), "norms": (nseg, torch.float32)})
    xa = O.gossip_step(x, mem, hat, GAMMA) if gossip else x
    d = (xa - hat).astype(F32)
    assert same_bits(W.x, xa) and same_bits(W.hat, hat) and same_bits(W.mem, mem)
    assert np.allclose(o.norms, O.l2_norms(d, lens), rtol=1e-6, atol=0)
    assert np.array_equal(o.packed, O.qsgd_pack(_qsgd_levels(d, lens, o.norms, 77, 5), d, Q))


for _l in (FLAT, SEG3):
    for _g in (False, True):
        case("qsgd", f"qsgd_compress-{len(_l)}seg-{'gossip' if _g else 'plain'}", ["qsgd_compress"])(
            lambda l=_l, g=_g: _qsgd_compress(l, g))


@case("qsgd", "qsgd_norms+quantize_range", ["qsgd_norms", "qsgd_quantize_range"])
def _qsgd_chunked():
    """The chunked sender: the norm pass with the consensus step, then two ranges quantized with its norms."""
    from chocosgd_amd import codec
    lens, n, nseg = SEG3, sum(SEG3), len(SEG3)
    x, hat, mem = state(n, 75)
    so = seg_table(lens)
    ranges = codec.qsgd_chunks(n, 2)
    assert len(ranges) == 2
    outs = {"norms": (nseg, torch.float32)}
    for i, (e0, e1) in enumerate(ranges):
        outs[f"part{i}"] = (codec.qsgd_packed_bytes(e1 - e0, Q), torch.uint8)

    def call(W):
        codec.qsgd_norms(W.x, xhat=W.hat, seg_off=so, nseg=nseg, gossip=(W.mem, GAMMA), out=W.norms)
        for i, (e0, e1) in enumerate(ranges):
            codec.qsgd_quantize_range(W.x, Q, W.norms, e0, e1, getattr(W, f"part{i}"), xhat=W.hat, seg_off=so,
                                      nseg=nseg, seed=11, offset=2)

    _, W, o = go("qsgd", "qsgd_norms+quantize_range", call, {"x": x, "hat": hat, "mem": mem}, outs=outs)
    xa = O.gossip_step(x, mem, hat, GAMMA)
    d = (xa - hat).astype(F32)
    assert same_bits(W.x, xa)
    assert np.allclose(o.norms, O.l2_norms(d, lens), rtol=1e-6, atol=0)
    lvl = _qsgd_levels(d, lens, o.norms, 11, 2)
    for i, (e0, e1) in enumerate(ranges):
        assert np.array_equal(getattr(o, f"part{i}"), O.qsgd_pack(lvl[e0:e1], d[e0:e1], Q)), i


def _qsgd_msgs(n, lens, nmsg, seed):
    """[(planes, norms)] packed on the host from chosen levels (test_gpu_receivers.qcase's recipe), their
    decodes, and the poison: other well-formed planes, norms of 1."""
    rng = np.random.default_rng([seed, n, nmsg])
    true, poison, dec = {}, {}, []
    for m in range(nmsg):
        lvl = rng.integers(0, S_LEVELS + 1, size=n)
        d = rng.standard_normal(n).astype(F32)
        norms = rng.uniform(0.5, 4.0, size=len(lens)).astype(F32)
        packed = O.qsgd_pack(lvl.astype(F32), d, Q)
        levels, neg = O.qsgd_unpack(packed, n, Q)
        dec.append(np.concatenate([O.qsgd_decode(levels[a:b], neg[a:b], norms[i], S_LEVELS, b - a)
                                   for i, (a, b) in enumerate(_bounds(lens))]))
        true[f"p{m}"], true[f"n{m}"] = packed, norms
        poison[f"p{m}"] = O.qsgd_pack(rng.integers(0, S_LEVELS + 1, size=n).astype(F32),
                                      rng.standard_normal(n).astype(F32), Q)
        poison[f"n{m}"] = np.ones(len(lens), F32)
    return true, poison, dec, rng


@case("qsgd", "qsgd_decode", ["qsgd_decode"])
def _qsgd_decode():
    from chocosgd_amd import codec
    lens, n = SEG3, sum(SEG3)
    true, poison, dec, _ = _qsgd_msgs(n, lens, 1, 1)
    so = seg_table(lens)
    ret, _, _ = go("qsgd", "qsgd_decode", lambda W: codec.qsgd_decode(W.p0, W.n0, n, Q, seg_off=so, nseg=len(lens)),
                   true, poison=poison)
    assert same_bits(ret, dec[0])


@case("qsgd", "qsgd_accumulate", ["qsgd_accumulate"])
def _qsgd_accumulate():
    from chocosgd_amd import codec
    lens, n, nmsg, slot = SEG3, sum(SEG3), 3, 1
    true, poison, dec, _ = _qsgd_msgs(n, lens, nmsg, 2)
    hat, mem = randn(n, 81), randn(n, 82)
    so, w = seg_table(lens), _weights(nmsg)
    _, W, _ = go("qsgd", "qsgd_accumulate",
                 lambda W: codec.qsgd_accumulate(_msgs_of(W, nmsg), w, slot, n, Q, W.mem, xhat_self=W.hat, seg_off=so,
                                                 nseg=len(lens)),
                 dict(true, hat=hat, mem=mem), poison=poison)
    h, m_ = hat.copy(), mem.copy()
    O.qsgd_accumulate(h, m_, dec, w, slot)
    assert same_bits(W.hat, h) and same_bits(W.mem, m_)


@case("qsgd", "qsgd_accumulate_range", ["qsgd_accumulate_range"])
def _qsgd_accumulate_range():
    """The chunked receiver: two ranges, each a self-contained message of its elements."""
    from chocosgd_amd import codec
    lens, n, nmsg, slot = SEG3, sum(SEG3), 3, 1
    rng = np.random.default_rng(83)
    ranges = codec.qsgd_chunks(n, 2)
    assert len(ranges) == 2
    so, w = seg_table(lens), _weights(nmsg)
    hat, mem = randn(n, 84), randn(n, 85)
    true, poison, dec = {"hat": hat, "mem": mem}, {}, []
    for m in range(nmsg):
        lvl, d = rng.integers(0, S_LEVELS + 1, size=n), rng.standard_normal(n).astype(F32)
        norms = rng.uniform(0.5, 4.0, size=len(lens)).astype(F32)
        true[f"n{m}"], poison[f"n{m}"] = norms, np.ones(len(lens), F32)
        for r, (e0, e1) in enumerate(ranges):
            true[f"p{m}r{r}"] = O.qsgd_pack(lvl[e0:e1].astype(F32), d[e0:e1], Q)
            poison[f"p{m}r{r}"] = O.qsgd_pack(rng.integers(0, S_LEVELS + 1, size=e1 - e0).astype(F32),
                                              rng.standard_normal(e1 - e0).astype(F32), Q)
        dec.append(np.concatenate([O.qsgd_decode(lvl[a:b], d[a:b] < 0, norms[i], S_LEVELS, b - a)
                                   for i, (a, b) in enumerate(_bounds(lens))]))

    def call(W):
        for r, (e0, e1) in enumerate(ranges):
            part = [(getattr(W, f"p{m}r{r}"), getattr(W, f"n{m}")) for m in range(nmsg)]
            codec.qsgd_accumulate_range(part, w, slot, n, Q, W.mem, e0, e1, xhat_self=W.hat, seg_off=so,
                                        nseg=len(lens))

    _, W, _ = go("qsgd", "qsgd_accumulate_range", call, true, poison=poison)
    h, m_ = hat.copy(), mem.copy()
    O.qsgd_accumulate(h, m_, dec, w, slot)
    assert same_bits(W.hat, h) and same_bits(W.mem, m_)


@case("qsgd", "qsgd_extrapolate", ["qsgd_extrapolate"])
def _qsgd_extrapolate():
    from chocosgd_amd import codec
    lens, n = SEG3, sum(SEG3)
    true, poison, dec, _ = _qsgd_msgs(n, lens, 1, 3)
    t0 = randn(n, 86)
    so = seg_table(lens)
    a, b = O.ecd_coeffs(3)
    _, W, _ = go("qsgd", "qsgd_extrapolate",
                 lambda W: codec.qsgd_extrapolate(W.p0, W.n0, n, Q, W.t, float(a), float(b), seg_off=so,
                                                  nseg=len(lens)),
                 dict(true, t=t0), poison=poison)
    assert same_bits(W.t, O.ecd_extrapolate(t0, dec[0], 3))


def _qsgd_recv(nmsg):
    """More than eight messages: the leading two go through qsgd_accumulate."""
    from chocosgd_amd import codec
    lens, n, slot = SEG3, sum(SEG3), 1
    true, poison, dec, _ = _qsgd_msgs(n, lens, nmsg, 4)
    x, hat, mem = state(n, 87)
    so, w = seg_table(lens), _weights(nmsg)
    _, W, o = go("qsgd", f"qsgd_recv_gossip_norms-{nmsg}",
                 lambda W: codec.qsgd_recv_gossip_norms(_msgs_of(W, nmsg), w, slot, W.x, W.mem, W.hat, GAMMA, Q,
                                                        seg_off=so, nseg=len(lens), out=W.norms),
                 dict(true, x=x, hat=hat, mem=mem), poison=poison, outs={"norms": (len(lens), torch.float32)})
    h, m_ = hat.copy(), mem.copy()
    O.qsgd_accumulate(h, m_, dec, w, slot)
    xa = O.gossip_step(x, m_, h, GAMMA)
    assert same_bits(W.hat, h) and same_bits(W.mem, m_) and same_bits(W.x, xa)
    assert np.allclose(o.norms, O.l2_norms((xa - h).astype(F32), lens), rtol=1e-6, atol=0)


for _m in (3, 10):
    case("qsgd", f"qsgd_recv_gossip_norms-{_m}", ["qsgd_recv_gossip_norms"])(lambda m=_m: _qsgd_recv(m))


# ---- gossip
@case("gossip", "gossip_step", ["gossip_step"])
def _gossip_step():
    from chocosgd_amd import codec
    n = 70_001
    x, hat, mem = state(n, 90)
    _, W, _ = go("gossip", "gossip_step", lambda W: codec.gossip_step(W.x, W.mem, W.hat, GAMMA),
                 {"x": x, "hat": hat, "mem": mem})
    assert same_bits(W.x, O.gossip_step(x, mem, hat, GAMMA)) and same_bits(W.hat, hat) and same_bits(W.mem, mem)


from _streams_param_cases import register as _register_param_cases  # noqa: E402

_register_param_cases(case, go)


# ------------------------------------------------------------------------------ the tests
@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_wrapper_on_a_delayed_side_stream(name):
    CASES[name].fn()
    ST.print_report(CASES[name].family)


# Diagnostics and documented synchronising readers only.
EXEMPT = {
    "TopkStatus.check": "diagnostic: reads the pinned host mirror of a workspace's status word; wait=True "
                        "synchronises by contract",
}


def launching_callables():
    """{name: source} of the public functions of codec.py and of the public methods of its public classes
    whose source passes `_stream(` -- itself, or through one of the module's private helpers that does
    (the plans' `_sgd` / `_adam`, `_mix_call`, `_ef_call`).  `_stream(` as a call of its own: the
    `torch.cuda.current_stream(` of the workspace management and of the synchronising diagnostics
    (`workspace`, `drop_workspace`, `topk_workspace_word`, `seg_*`) is not one.  The public one-line
    wrappers over a plan method (`params_sgd`, `params_sgd_master`, `params_sgd_flatgrad`, `params_adam`,
    `params_adam_master`, `params_sqnorm`, `params_consensus`, `params_ef`) fill the tables and call the
    method; they are not enumerated, the plan methods they call are."""
    from chocosgd_amd import codec
    public, private = {}, {}
    for name, obj in vars(codec).items():
        if getattr(obj, "__module__", None) != codec.__name__:
            continue
        if inspect.isfunction(obj):
            (private if name.startswith("_") else public)[name] = inspect.getsource(obj)
        elif inspect.isclass(obj) and not name.startswith("_"):
            for mname, m in vars(obj).items():
                if inspect.isfunction(m) and not mname.startswith("__"):
                    (private if mname.startswith("_") else public)[f"{name}.{mname}"] = inspect.getsource(m)
    passes = re.compile(r"(?<![A-Za-z0-9_])_stream\(")
    helpers = {k.split(".")[-1] for k, src in private.items() if passes.search(src)} - {"_stream"}
    assert helpers == {"_sgd", "_adam", "_mix_call", "_ef_call"}, helpers
    calls = re.compile(r"(?<![A-Za-z0-9_])(" + "|".join(sorted(helpers | {"_stream"})) + r")\(")
    return {k: src for k, src in public.items() if calls.search(src)}


def test_every_launching_wrapper_is_in_the_table():
    """Host: the table grows with the library.  A public callable that hands the library a stream is
    covered by a case or exempt for a stated reason; nothing is both, and nothing listed has gone."""
    launching = launching_callables()
    assert len(launching) >= 40, sorted(launching)
    covered = {c for v in CASES.values() for c in v.covers}
    missing = sorted(set(launching) - covered - set(EXEMPT))
    assert not missing, f"launching wrappers without a stream case: {missing}"
    assert not covered & set(EXEMPT), sorted(covered & set(EXEMPT))
    assert set(EXEMPT) <= set(launching), f"exempt, but not launching: {sorted(set(EXEMPT) - set(launching))}"
    from chocosgd_amd import codec
    for name in sorted(covered | set(EXEMPT)):
        obj = codec
        for part in name.split("."):
            obj = getattr(obj, part)  # a renamed wrapper fails here
    for name, reason in EXEMPT.items():
        assert reason and (name.startswith(("profile_", "seg_", "topk_workspace_word", "topk_fallback_count",
                                            "TopkStatus", "check_topk_status"))
                           or "workspace" in name), name
