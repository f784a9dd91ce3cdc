"""choco_params_ef and choco_sign_local_residual, host side (no GPU): the launch count rule and
the argument checks, made before any HIP call -- every refusal returns CHOCO_ERR_INVALID with a
message that names the fault, and counts no launch."""
import ctypes

import pytest
import torch

CAP = 128  # tensors per launch (ef.hip kEfCap)
ERR_INVALID = -1  # CHOCO_ERR_INVALID
F32, BF16, F16 = 0, 1, 2
ACCUM, APPLY, DIV, SCALE = 1, 2, 4, 8


@pytest.fixture(scope="module")
def lib():
    from chocosgd_amd import _lib
    return _lib.load()


def test_launches_rule(lib):
    from chocosgd_amd import codec
    for nseg, want in [(0, 0), (1, 1), (CAP, 1), (CAP + 1, 2), (2 * CAP + 1, 3)]:
        assert lib.choco_params_ef_launches(nseg) == want, nseg
        assert codec.params_ef_launches(nseg) == want
    assert lib.choco_params_ef_launches(-3) == 0
    assert lib.choco_params_ef_launches(161) == 2  # ResNet-50


def _call(lib, p=(0x1000, 0x1100), lens=(4, 4), dts=(F32, BF16), nseg=None, flat=0x40000, n=8, mode=APPLY, lr=0.1,
          divisor=3.0, null=(), msg=None):
    """One call with host tables built from the lists; the made-up device pointers are never
    dereferenced (every case here is rejected before the first launch)."""
    arr = lambda ct, vals: (ct * max(len(vals), 1))(*vals)  # noqa: E731
    tabs = {"params": arr(ctypes.c_void_p, p), "lens": arr(ctypes.c_int64, lens), "dtypes": arr(ctypes.c_int32, dts)}
    t = {nm: (None if nm in null else tab) for nm, tab in tabs.items()}
    return lib.choco_params_ef(t["params"], t["lens"], t["dtypes"], len(lens) if nseg is None else nseg,
                               ctypes.c_void_p(flat), n, mode, lr, divisor, None)


BAD = {
    **{f"null {t}": dict(null=(t,), msg="null table") for t in ["params", "lens", "dtypes"]},
    "nseg zero": dict(nseg=0, msg="nseg"),
    "nseg negative": dict(nseg=-2, msg="nseg"),
    "negative length": dict(lens=(-4, 12), msg="negative length"),
    "sum below n": dict(n=9, msg="add up"),
    "sum above n": dict(n=7, msg="add up"),
    "dtype 3": dict(dts=(F32, 3), msg="dtype"),
    "dtype -1": dict(dts=(-1, F32), msg="dtype"),
    "unknown mode bit": dict(mode=16 | APPLY, msg="unknown mode"),
    "neither ACCUM nor APPLY": dict(mode=0, msg="exactly one"),
    "DIV alone": dict(mode=DIV, msg="exactly one"),
    "both ACCUM and APPLY": dict(mode=ACCUM | APPLY, msg="exactly one"),
    "DIV with ACCUM": dict(mode=ACCUM | DIV, msg="belong to APPLY"),
    "SCALE with ACCUM": dict(mode=ACCUM | SCALE, msg="belong to APPLY"),
    "null flat": dict(flat=0, msg="flat is null"),
    "null flat with ACCUM": dict(flat=0, mode=ACCUM, msg="flat is null"),
    "null param": dict(p=(0x1000, 0), msg="null param"),
    "null param with ACCUM": dict(p=(0, 0x1100), mode=ACCUM, msg="null param"),
    "flat at 2 mod 4": dict(flat=0x40002, msg="4-byte"),
    "fp32 param at 2 mod 4": dict(p=(0x1002, 0x1100), msg="aligned"),
    "bf16 param at odd byte": dict(p=(0x1000, 0x1101), msg="aligned"),
    "fp16 param at odd byte": dict(dts=(F32, F16), p=(0x1000, 0x1101), mode=ACCUM, msg="aligned"),
    "divisor zero": dict(mode=APPLY | DIV, divisor=0.0, msg="divisor"),
    "divisor zero as a float": dict(mode=APPLY | DIV, divisor=1e-60, msg="divisor"),
    "divisor inf": dict(mode=APPLY | DIV | SCALE, divisor=float("inf"), msg="divisor"),
    "divisor nan": dict(mode=APPLY | DIV, divisor=float("nan"), msg="divisor"),
    "lr inf": dict(mode=APPLY | SCALE, lr=float("inf"), msg="lr must be finite"),
    "lr nan": dict(mode=APPLY | DIV | SCALE, lr=float("nan"), msg="lr must be finite"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_arguments_are_rejected(lib, case):
    from chocosgd_amd import _lib, codec
    before = codec.launch_count("param_ef_kernel")
    assert _call(lib, **BAD[case]) == ERR_INVALID, case
    err = _lib.last_error()
    assert err != "" and BAD[case]["msg"] in err, (case, err)
    assert codec.launch_count("param_ef_kernel") == before


def _residual(lib, x=0x10000, n=64, seg_off=None, nseg=1, norms=0x20000, local=0x30000, resid=0x40000):
    so = (ctypes.c_int64 * len(seg_off))(*seg_off) if seg_off is not None else None
    return lib.choco_sign_local_residual(ctypes.c_void_p(x), n, so, nseg, ctypes.c_void_p(norms),
                                         ctypes.c_void_p(local), ctypes.c_void_p(resid), None)


BAD_RESIDUAL = {
    "null x": dict(x=0, msg="null pointer"),
    "null norms": dict(norms=0, msg="null pointer"),
    "null resid_out": dict(resid=0, msg="null pointer"),
    "n zero": dict(n=0, msg="n out of range"),
    "n = 2^31": dict(n=2 ** 31, msg="n out of range"),
    "nseg zero": dict(nseg=0, msg="seg_off"),
    "two segments without seg_off": dict(nseg=2, msg="seg_off"),
    "x at 2 mod 4": dict(x=0x10002, msg="4-byte"),
    "local_out at 2 mod 4": dict(local=0x30002, msg="4-byte"),
    "resid_out at 2 mod 4": dict(resid=0x40002, msg="4-byte"),
    "local_out is x": dict(local=0x10000, msg="local_out aliases"),
    "local_out overlaps x": dict(local=0x10000 + 4 * 63, msg="local_out aliases"),
    "local_out is resid_out": dict(local=0x40000, msg="local_out aliases"),
    "local_out is x, in place": dict(local=0x10000, resid=0x10000, msg="local_out aliases"),
    "resid_out overlaps x": dict(resid=0x10000 + 4 * 8, msg="resid_out overlaps"),
}


@pytest.mark.parametrize("case", sorted(BAD_RESIDUAL))
def test_residual_invalid_arguments_are_rejected(lib, case):
    from chocosgd_amd import _lib, codec
    before = codec.launch_count("sign_local_residual")
    kw = dict(BAD_RESIDUAL[case])
    msg = kw.pop("msg")
    assert _residual(lib, **kw) == ERR_INVALID, case
    err = _lib.last_error()
    assert err != "" and msg in err, (case, err)
    assert codec.launch_count("sign_local_residual") == before


def test_python_wrappers_refuse_cpu_tensors():
    from chocosgd_amd import codec
    with pytest.raises(RuntimeError, match="ROCm device"):
        codec.params_ef([torch.zeros(8)], torch.zeros(8), codec.EF_ACCUM)
    with pytest.raises(RuntimeError, match="ROCm device"):
        codec.sign_local_residual(torch.zeros(8), torch.zeros(1))


def test_mode_constants_match_the_header():
    import os
    import re
    from conftest import ROOT
    from chocosgd_amd import codec
    src = open(os.path.join(ROOT, "include", "choco_codec.h")).read()
    hdr = {k: int(v) for k, v in re.findall(r"#define CHOCO_EF_([A-Z]+) (\d+)", src)}
    assert hdr == {"ACCUM": codec.EF_ACCUM, "APPLY": codec.EF_APPLY, "DIV": codec.EF_DIV, "SCALE": codec.EF_SCALE}
