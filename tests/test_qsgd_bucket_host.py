"""Bucketed QSGD, host side (no GPU): the message size, and every refusal -- each entry point checks
its arguments before the first launch and without a HIP call (fake pointers, one fault per case), and
the drop-ins refuse by name what the bucketed op does not do."""
import pytest

from chocosgd_amd import _lib

ERR_INVALID = -1  # CHOCO_ERR_INVALID
N = 4096
X, MEM, XHAT, OUT, DENSE, U = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
MSG0 = 0x1000000  # message i: MSG0 + i * 0x10000


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_packed_bytes(lib):
    for n in (1, 7, 512, 513, 27141, 100_000_000):
        for q, cw in ((1, 1), (3, 4), (4, 4), (8, 8), (9, 16), (16, 16)):
            for B in (128, 256, 512, 1024, 2048):
                nb, groups = -(-n // B), -(-n // 8)
                want = (4 * nb + 15) // 16 * 16 + (groups * cw + 15) // 16 * 16 + (groups + 15) // 16 * 16
                assert lib.choco_qsgd_bucket_packed_bytes(n, q, B) == want
                assert want == (4 * nb + 15) // 16 * 16 + lib.choco_qsgd_packed_bytes(n, q)
    for bad in ((0, 4, 512), (10, 0, 512), (10, 17, 512), (10, 4, 500), (10, 4, 64), (10, 4, 4096)):
        assert lib.choco_qsgd_bucket_packed_bytes(*bad) == 0


def _call(lib, fn, **over):
    s = dict(x=X, mem=MEM, xhat=XHAT, out=OUT, dense=DENSE, u=U, n=N, q=4, B=512, nmsg=2, slot=0,
             msgs=[MSG0, MSG0 + 0x10000], lists=True)
    s.update(over)
    pp, keep1 = _lib.ptr_array(s["msgs"])
    ww, keep2 = _lib.f32_array([0.5] * len(s["msgs"]))
    if not s["lists"]:
        pp = ww = None
    tail = (s["n"], s["q"], s["B"], 0, s["u"], 1, 0, s["out"])
    if fn == "compress":
        return lib.choco_qsgd_bucket_compress(s["x"], s["xhat"], *tail, s["dense"], None)
    if fn == "gossip_compress":
        return lib.choco_gossip_qsgd_bucket_compress(s["x"], s["mem"], s["xhat"], 0.5, *tail, s["dense"], None)
    if fn == "decode":
        return lib.choco_qsgd_bucket_decode(s["msgs"][0], s["n"], s["q"], s["B"], 0, s["out"], None)
    if fn == "accumulate":
        return lib.choco_qsgd_bucket_decompress_accumulate(pp, ww, s["nmsg"], s["slot"], s["n"], s["q"], s["B"], 0,
                                                           s["xhat"], s["mem"], None)
    return lib.choco_qsgd_bucket_recv_gossip_compress(pp, ww, s["nmsg"], s["slot"], s["x"], s["mem"], s["xhat"], 0.5,
                                                      *tail, None)


COMMON = {"n = 0": (dict(n=0), "out of range"), "q = 0": (dict(q=0), "q must be in"),
          "q = 17": (dict(q=17), "q must be in"), "bucket 500": (dict(B=500), "bucket must be one of"),
          "bucket 4096": (dict(B=4096), "bucket must be one of")}
SEND = {"null x": (dict(x=None), "null"), "null message": (dict(out=None), "null"),
        "misaligned x": (dict(x=X + 4), "aligned"), "misaligned message": (dict(out=OUT + 8), "aligned"),
        "misaligned u_in": (dict(u=U + 4), "aligned"), "message inside x": (dict(out=X + 64), "alias"),
        "x_hat inside message": (dict(xhat=OUT + 16), "alias")}
MSGS = {"nmsg 0": (dict(nmsg=0), "nmsg"), "nmsg 9": (dict(nmsg=9), "nmsg"), "self_slot == nmsg": (dict(slot=2), "self_slot"),
        "null lists": (dict(lists=False), "null"), "null message in the list": (dict(msgs=[MSG0, 0]), "null"),
        "misaligned list message": (dict(msgs=[MSG0, MSG0 + 0x10008]), "aligned"), "null memory": (dict(mem=None), "null"),
        "misaligned memory": (dict(mem=MEM + 4), "aligned")}
ENTRY = {
    "compress": {**COMMON, **SEND, "misaligned dense_out": (dict(dense=DENSE + 4), "aligned")},
    "gossip_compress": {**COMMON, **SEND, "null memory": (dict(mem=None), "null"),
                        "message inside memory": (dict(out=MEM + 64), "alias")},
    "decode": {**COMMON, "null out": (dict(out=None), "null"), "null message": (dict(msgs=[0]), "null"),
               "misaligned message": (dict(msgs=[MSG0 + 8]), "aligned"), "misaligned out": (dict(out=OUT + 4), "aligned")},
    "accumulate": {**COMMON, **MSGS},
    "recv_gossip_compress": {**COMMON, **MSGS, "null x": (dict(x=None), "null"),
                             "null message_out": (dict(out=None), "null"),
                             "output inside message 1": (dict(out=MSG0 + 0x10000 + 64), "alias"),
                             "output inside memory": (dict(out=MEM + 1024), "alias")},
}
CASES = [(fn, case) for fn in ENTRY for case in ENTRY[fn]]


@pytest.mark.parametrize("fn,case", CASES, ids=[f"{f}-{c}" for f, c in CASES])
def test_single_fault_is_rejected_before_any_launch(lib, fn, case):
    over, word = ENTRY[fn][case]
    assert _call(lib, fn, **over) == ERR_INVALID
    assert word in _lib.last_error(), _lib.last_error()


ARGS = dict(aggregator=None, comm_device="gpu", compress_ratio=0.9, is_biased=False, backend="nccl", use_ipc=False)


@pytest.mark.parametrize("module,cls,kw,exc,word", [
    ("parallel_choco", "CHOCOCompressor", dict(quantize_level=4, exchange_chunks=2), RuntimeError, "exchange_chunks"),
    ("parallel_choco", "CHOCOCompressor", dict(quantize_level=32), NotImplementedError, "quantize_level = 32"),
    ("parallel_choco", "CHOCOCompressor", dict(quantize_level=4, bucket_size=300), RuntimeError, "bucket_size"),
    ("dcd", "DCDCompressor", dict(quantize_level=4), NotImplementedError, "bucketed"),
    ("ecd", "ECDCompressor", dict(quantize_level=4), NotImplementedError, "bucketed"),
    ("deep_squeeze", "DeepSqueezeCompressor", dict(quantize_level=4, rank=0, consensus_stepsize=0.5), NotImplementedError,
     "bucketed"),
])
def test_drop_ins_refuse_by_name(module, cls, kw, exc, word):
    import importlib
    ctor = getattr(importlib.import_module("chocosgd_amd." + module), cls)
    with pytest.raises(exc, match=word):
        ctor(comm_op="quantize_qsgd_bucket", **ARGS, **kw)


def test_quantization_compressor_refuses_the_passthrough():
    import torch
    from chocosgd_amd.sparsification import QuantizationCompressor
    with pytest.raises(NotImplementedError, match="quantize_level = 32"):
        QuantizationCompressor().compress(torch.zeros(8), "quantize_qsgd_bucket", 32, False)
