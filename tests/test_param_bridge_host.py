"""Parameter bridge, host side (no GPU): the launch count rule, the argument checks of
choco_params_pack / choco_params_unpack (made before any HIP call), and the per-tensor loop
path of flatten / TensorBuffer, which CPU tensors keep."""
import ctypes

import pytest
import torch

from chocosgd_amd import _lib, codec
from chocosgd_amd.tensor_buffer import TensorBuffer, flatten

CAP = 192  # tensors per launch (params.hip kParamCap)
ERR_INVALID = -1  # CHOCO_ERR_INVALID
F32, BF16, F16 = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_launches_rule(lib):
    for nseg in [1, CAP - 1, CAP, CAP + 1, 3000]:
        assert lib.choco_params_launches(nseg) == -(-nseg // CAP), nseg
        assert codec.params_launches(nseg) == -(-nseg // CAP)
    assert lib.choco_params_launches(161) == 1  # ResNet-50 in one launch


def _call(lib, fn, ptrs, lens, dts, n, flat=0x10000, nseg=None, null=(), msg=None):
    """One call with host tables built from the lists; the pointers are never dereferenced
    (every case here is rejected before the first launch)."""
    k = len(ptrs)
    a_p = (ctypes.c_void_p * max(k, 1))(*ptrs)
    a_l = (ctypes.c_int64 * max(k, 1))(*lens)
    a_d = (ctypes.c_int32 * max(k, 1))(*dts)
    args = [None if "ptrs" in null else a_p, None if "lens" in null else a_l, None if "dtypes" in null else a_d]
    return getattr(lib, fn)(*args, k if nseg is None else nseg, ctypes.c_void_p(flat), n, None)


BAD = {
    "null ptrs": dict(ptrs=[0x1000], lens=[4], dts=[F32], n=4, null=("ptrs",), msg="null table"),
    "null lens": dict(ptrs=[0x1000], lens=[4], dts=[F32], n=4, null=("lens",), msg="null table"),
    "null dtypes": dict(ptrs=[0x1000], lens=[4], dts=[F32], n=4, null=("dtypes",), msg="null table"),
    "nseg zero": dict(ptrs=[0x1000], lens=[4], dts=[F32], n=4, nseg=0, msg="nseg"),
    "nseg negative": dict(ptrs=[0x1000], lens=[4], dts=[F32], n=4, nseg=-3, msg="nseg"),
    "negative length": dict(ptrs=[0x1000, 0x2000], lens=[-4, 8], dts=[F32, F32], n=4, msg="negative length"),
    "dtype 3": dict(ptrs=[0x1000], lens=[4], dts=[3], n=4, msg="dtype"),
    "dtype -1": dict(ptrs=[0x1000], lens=[4], dts=[-1], n=4, msg="dtype"),
    "sum below n": dict(ptrs=[0x1000, 0x2000], lens=[4, 4], dts=[F32, BF16], n=9, msg="add up"),
    "sum above n": dict(ptrs=[0x1000, 0x2000], lens=[4, 4], dts=[F32, BF16], n=7, msg="add up"),
    "n = 2^31": dict(ptrs=[0x1000], lens=[2 ** 31], dts=[F32], n=2 ** 31, msg="2^31"),
    "null tensor": dict(ptrs=[0x1000, 0], lens=[4, 4], dts=[F32, F32], n=8, msg="null pointer"),
    "fp32 at 2 mod 4": dict(ptrs=[0x1002], lens=[4], dts=[F32], n=4, msg="aligned"),
    "bf16 at odd byte": dict(ptrs=[0x1001], lens=[4], dts=[BF16], n=4, msg="aligned"),
    "fp16 at odd byte": dict(ptrs=[0x1000, 0x2003], lens=[4, 4], dts=[F32, F16], n=8, msg="aligned"),
}


@pytest.mark.parametrize("fn", ["choco_params_pack", "choco_params_unpack"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_arguments_are_rejected(lib, fn, case):
    assert _call(lib, fn, **BAD[case]) == ERR_INVALID, case
    err = _lib.last_error()
    assert err != "" and BAD[case]["msg"] in err, (case, err)


def _loop_flatten(tensors, dtype):
    out = torch.empty(sum(t.numel() for t in tensors), dtype=dtype)
    o = 0
    for t in tensors:
        out[o:o + t.numel()] = t.reshape(-1)
        o += t.numel()
    return out


def _cpu_tensors(dtype):
    g = torch.Generator().manual_seed(3)
    shapes = [(3, 5), (1,), (0,), (7,), (2, 2, 2)]
    if dtype == torch.int64:
        return [torch.randint(-2 ** 40, 2 ** 40, s, generator=g, dtype=dtype) for s in shapes]
    return [(torch.randn(s, generator=g) * 100).to(dtype) for s in shapes]


@pytest.mark.parametrize("dtype", [torch.int64, torch.bfloat16, torch.float32])
def test_cpu_flatten_and_unpack_unchanged(dtype):
    ts = _cpu_tensors(dtype)
    want = _loop_flatten(ts, dtype)
    flat = flatten(ts)
    assert flat.dtype == dtype and flat.device.type == "cpu" and torch.equal(flat, want)
    assert torch.equal(flatten(ts, dtype=None), want)
    tb = TensorBuffer(ts)
    assert tb.buffer.dtype == dtype and torch.equal(tb.buffer, want)
    assert [tuple(tb[i].shape) for i in range(len(tb))] == [tuple(t.shape) for t in ts]
    outs = [torch.zeros_like(t) for t in ts]
    tb.unpack(outs)
    for o, t in zip(outs, ts):
        assert torch.equal(o, t)
    # shapes= with sizes of its own: the loop broadcasts each tensor into its slot
    one = [torch.full((1,), 7, dtype=dtype), torch.full((1,), 9, dtype=dtype)]
    got = flatten(one, shapes=[(None, 3), (None, 2)])
    assert got.tolist() == [7, 7, 7, 9, 9]


def test_cpu_flatten_dtype_widens_bf16_through_the_loop():
    ts = _cpu_tensors(torch.bfloat16)
    flat = flatten(ts, dtype=torch.float32)
    assert flat.dtype == torch.float32 and flat.device.type == "cpu"
    assert torch.equal(flat, _loop_flatten(ts, torch.float32))
    assert torch.equal(flat, torch.cat([t.reshape(-1).float() for t in ts]))
    tb = TensorBuffer(ts, dtype=torch.float32)
    assert tb.buffer.dtype == torch.float32
    tb.buffer.mul_(1.0 + 2.0 ** -9)  # off the bf16 grid: unpack must round
    outs = [torch.zeros_like(t) for t in ts]
    tb.unpack(outs)
    for i, (o, t) in enumerate(zip(outs, ts)):
        assert o.dtype == torch.bfloat16 and torch.equal(o, tb[i].to(torch.bfloat16))
