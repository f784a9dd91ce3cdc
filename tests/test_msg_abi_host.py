"""Multi-message entry points, host side (no GPU): every argument check is made before the
first HIP call, returns CHOCO_ERR_INVALID and leaves a text that names the fault.  The
pointers are fake and never dereferenced: each case has exactly one fault."""
import ctypes

import pytest

from chocosgd_amd import _lib

ERR_INVALID = -1  # CHOCO_ERR_INVALID
N = 4096          # elements: 128 sign words; under one QSGD stream tile, so [0, N) is the only valid range
X, MEM, XHAT, OUT, NORMS_OUT, WS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
MSG0, NORM0 = 0x1000000, 0x2000000  # message q: MSG0 + q * 0x10000, its norms NORM0 + q * 0x100
SEG_OFF = 0x700000
WS_BYTES = 1 << 30


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _state(**over):
    s = dict(nmsg=2, self_slot=0, n=N, nseg=1, seg_off=None, q=4, e0=0, e1=N, null_list=None, msgs=None,
             norms=None, memory=MEM, out=OUT)
    s.update(over)
    k = max(s["nmsg"], 1)
    if s["msgs"] is None:
        s["msgs"] = [MSG0 + i * 0x10000 for i in range(k)]
    if s["norms"] is None:
        s["norms"] = [NORM0 + i * 0x100 for i in range(k)]
    return s


def _lists(s, names=("packed", "norms", "weights")):
    k = len(s["msgs"])
    packed, keep_p = _lib.ptr_array(s["msgs"])
    norms, keep_n = _lib.ptr_array(s["norms"])
    weights, keep_w = _lib.f32_array([0.5] * k)
    got = dict(packed=packed, norms=norms, weights=weights)
    if s["null_list"]:
        got[s["null_list"]] = None
    return [got[n] for n in names], (keep_p, keep_n, keep_w)


def _sign_acc(lib, s):
    (p, nr, w), keep = _lists(s)
    return lib.choco_sign_decompress_accumulate(p, nr, w, s["nmsg"], s["self_slot"], s["n"], s["seg_off"], s["nseg"],
                                                XHAT, s["memory"], None, 0, None)


def _sign_axpy(lib, s):
    (p, nr, w), keep = _lists(s)
    return lib.choco_sign_decompress_axpy(p, nr, w, s["nmsg"], s["n"], s["seg_off"], s["nseg"], 0, s["memory"], None)


def _sign_recv(lib, s):
    (p, nr, w), keep = _lists(s)
    return lib.choco_sign_recv_gossip_compress(p, nr, w, s["nmsg"], s["self_slot"], X, s["memory"], XHAT, 0.5, s["n"],
                                               s["seg_off"], s["nseg"], s["out"], NORMS_OUT, WS, WS_BYTES, None)


def _qsgd_acc(lib, s):
    (p, nr, w), keep = _lists(s)
    return lib.choco_qsgd_decompress_accumulate(p, nr, w, s["nmsg"], s["self_slot"], s["n"], s["seg_off"], s["nseg"],
                                                s["q"], 0, XHAT, s["memory"], None)


def _qsgd_range(lib, s):
    (p, nr, w), keep = _lists(s)
    return lib.choco_qsgd_decompress_accumulate_range(p, nr, w, s["nmsg"], s["self_slot"], s["n"], s["seg_off"],
                                                      s["nseg"], s["q"], 0, s["e0"], s["e1"], XHAT, s["memory"], None)


def _qsgd_recv(lib, s):
    (p, nr, w), keep = _lists(s)
    return lib.choco_qsgd_recv_gossip_norms(p, nr, w, s["nmsg"], s["self_slot"], X, s["memory"], XHAT, 0.5, s["n"],
                                            s["seg_off"], s["nseg"], s["q"], 0, NORMS_OUT, WS, WS_BYTES, None)


def _sparse_multi(lib, s):
    (vals, idxs, w), keep = _lists(s)  # values in the `packed` role, indices in the `norms` role
    ks, keep_k = _lib.i64_array([16] * len(s["msgs"]))
    return lib.choco_sparse_accumulate_multi(vals, idxs, ks, w, s["nmsg"], s["self_slot"], XHAT, s["memory"], s["n"],
                                             None, 0, None, None)


# single-fault inputs: name -> (state overrides, the word today's text carries)
NMSG = {
    "nmsg 0": (dict(nmsg=0), "nmsg"),
    "nmsg 9": (dict(nmsg=9), "nmsg"),
    "null packed list": (dict(null_list="packed"), "null pointer"),
    "null norms list": (dict(null_list="norms"), "null pointer"),
    "null weights": (dict(null_list="weights"), "null pointer"),
    "null message": (dict(msgs=[MSG0, 0]), "null"),
    "null message norms": (dict(norms=[NORM0, 0]), "null"),
}
SELF = {"self_slot == nmsg": (dict(self_slot=2), "self_slot")}
FLAT = {
    "n = 0": (dict(n=0, e1=0), "out of range"),
    "nseg 2, null seg_off": (dict(nseg=2), "seg_off"),
    "misaligned buffer": (dict(memory=MEM + 4), "aligned"),
}
QLEVEL = {
    "q = 0": (dict(q=0), "q must be in"),
    "q = 17": (dict(q=17), "q must be in"),
    "misaligned message": (dict(msgs=[MSG0, MSG0 + 0x10008]), "aligned"),
}
RANGE = {
    "e0 off the tile grid": (dict(e0=8), "range"),
    "e1 past n": (dict(e1=N + 1), "range"),
    "empty range": (dict(e0=0, e1=0), "range"),
}
ALIAS = {
    "output inside message 1": (dict(out=MSG0 + 0x10000 + 64), "alias"),
    "message 0 inside output": (dict(out=MSG0 - 64), "alias"),
}

ENTRY = {
    "choco_sign_decompress_accumulate": (_sign_acc, {**NMSG, **SELF, **FLAT}),
    "choco_sign_decompress_axpy": (_sign_axpy, {**NMSG, **FLAT}),
    "choco_sign_recv_gossip_compress": (_sign_recv, {**NMSG, **SELF, **FLAT, **ALIAS}),
    "choco_qsgd_decompress_accumulate": (_qsgd_acc, {**NMSG, **SELF, **FLAT, **QLEVEL}),
    "choco_qsgd_decompress_accumulate_range": (_qsgd_range, {**NMSG, **SELF, **FLAT, **QLEVEL, **RANGE}),
    "choco_qsgd_recv_gossip_norms": (_qsgd_recv, {**NMSG, **SELF, **FLAT, **QLEVEL}),
    # (no segments, no alignment demand: the unaligned kernel takes those buffers)
    "choco_sparse_accumulate_multi": (_sparse_multi, {**NMSG, **SELF, "n = 0": (dict(n=0), "n must be positive")}),
}
CASES = [(fn, case) for fn in sorted(ENTRY) for case in sorted(ENTRY[fn][1])]


@pytest.mark.parametrize("fn,case", CASES, ids=[f"{f[6:]}-{c}" for f, c in CASES])
def test_single_fault_is_rejected_before_any_launch(lib, fn, case):
    call, cases = ENTRY[fn]
    over, word = cases[case]
    assert call(lib, _state(**over)) == ERR_INVALID, (fn, case)
    err = _lib.last_error()
    assert word in err, (fn, case, err)
