"""The MX wire, host side (no GPU): the message size and the refusals by name (fake pointers: no HIP call)."""
import pytest

from chocosgd_amd import _lib

X, MEM, XHAT, OUT = 0x100000, 0x200000, 0x300000, 0x400000
MSG0 = 0x1000000


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_packed_bytes(lib):
    for n in (1, 7, 31, 33, 8192, 8193, 27141, 100_000_000):
        for q in (4, 8):
            assert lib.choco_mx_packed_bytes(n, q) == (-(-n // 32) + 15) // 16 * 16 + ((n * q + 7) // 8 + 15) // 16 * 16
    for bad in ((0, 4), (10, 0), (10, 5), (10, 16), (2 ** 31, 8)):
        assert lib.choco_mx_packed_bytes(*bad) == 0


@pytest.mark.parametrize("over,word", [(dict(q=5), "q must be 4"), (dict(n=0), "out of range"), (dict(x=None), "null"),
                                       (dict(out=OUT + 8), "aligned"), (dict(out=X + 64), "alias"),
                                       (dict(nmsg=9), "nmsg"), (dict(out=MSG0 + 64), "alias")])
def test_library_refuses_before_any_launch(lib, over, word):
    s = dict(x=X, out=OUT, n=4096, q=4, nmsg=2)
    s.update(over)
    pp, _k1 = _lib.ptr_array([MSG0, MSG0 + 0x10000])
    ww, _k2 = _lib.f32_array([0.5, 0.5])
    tail = (s["n"], s["q"], 1, 1, 0, s["out"])
    calls = [lib.choco_mx_recv_gossip_compress(pp, ww, s["nmsg"], 0, s["x"], MEM, XHAT, 0.5, *tail, None)]
    if "nmsg" not in over and s["out"] != MSG0 + 64:
        calls += [lib.choco_mx_compress(s["x"], XHAT, *tail, None, None),
                  lib.choco_gossip_mx_compress(s["x"], MEM, XHAT, 0.5, *tail, None, None)]
    for rc in calls:
        assert rc == -1 and word in _lib.last_error(), _lib.last_error()  # CHOCO_ERR_INVALID


ARGS = dict(aggregator=None, comm_op="quantize_mx", comm_device="gpu", compress_ratio=0.9, is_biased=False,
            backend="nccl", use_ipc=False)


@pytest.mark.parametrize("module,cls,kw,exc,word", [
    ("parallel_choco", "CHOCOCompressor", dict(quantize_level=4, exchange_chunks=2), RuntimeError, "exchange_chunks"),
    ("parallel_choco", "CHOCOCompressor", dict(quantize_level=5), RuntimeError, "quantize_level 4"),
    ("parallel_choco", "CHOCOCompressor", dict(quantize_level=32), RuntimeError, "quantize_level 4"),
    ("dcd", "DCDCompressor", dict(quantize_level=4), NotImplementedError, "quantize_mx"),
    ("ecd", "ECDCompressor", dict(quantize_level=4), NotImplementedError, "quantize_mx"),
    ("deep_squeeze", "DeepSqueezeCompressor", dict(quantize_level=4, rank=0, consensus_stepsize=0.5), NotImplementedError,
     "quantize_mx"),
])
def test_drop_ins_refuse_by_name(module, cls, kw, exc, word):
    import importlib
    ctor = getattr(importlib.import_module("chocosgd_amd." + module), cls)
    with pytest.raises(exc, match=word):
        ctor(**ARGS, **kw)
