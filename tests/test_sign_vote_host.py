"""choco_sign_vote and choco_params_sign_step, host side (no GPU): the argument checks, made
before any HIP call -- every refusal returns CHOCO_ERR_INVALID with a message that names the fault
and counts no launch -- and the launch count rule."""
import ctypes

import pytest

CAP = 176  # tensors per launch (signstep.hip kStepCap)
ERR_INVALID = -1  # CHOCO_ERR_INVALID
F32, BF16 = 0, 1


@pytest.fixture(scope="module")
def lib():
    from chocosgd_amd import _lib
    return _lib.load()


def _arr(ct, vals):
    return (ct * max(len(vals), 1))(*vals)


def _vote(lib, voters=(0x1000, 0x2000, 0x3000), nvoters=None, nwords=8, out=0x4000):
    """The made-up device pointers are never dereferenced: every case is rejected before the launch."""
    return lib.choco_sign_vote(_arr(ctypes.c_void_p, voters), len(voters) if nvoters is None else nvoters, nwords,
                               ctypes.c_void_p(out), None)


def _step(lib, p=(0x1000, 0x1100), lens=(4, 4), dts=(F32, BF16), lr=(0.1, 0.2), verdict=0x4000, n=8):
    return lib.choco_params_sign_step(_arr(ctypes.c_void_p, p), _arr(ctypes.c_int64, lens), _arr(ctypes.c_int32, dts),
                                      _arr(ctypes.c_double, lr), len(lens), ctypes.c_void_p(verdict), n, None)


BAD = {
    "no voters": (_vote, dict(nvoters=0), "nvoters"),
    "65 voters": (_vote, dict(voters=(0x1000,) * 65), "nvoters"),
    "a null voter": (_vote, dict(voters=(0x1000, 0, 0x3000)), "voter 1: null"),
    "a voter at 2 mod 4": (_vote, dict(voters=(0x1000, 0x2002)), "voter 1: must be 4-byte"),
    "negative nwords": (_vote, dict(nwords=-1), "nwords"),
    "nwords above 2^26": (_vote, dict(nwords=2 ** 26 + 1), "nwords"),
    "null out": (_vote, dict(out=0), "null pointer"),
    "lens not summing to n": (_step, dict(n=9), "add up"),
    "dtype 3": (_step, dict(dts=(F32, 3)), "dtype"),
    "lr inf": (_step, dict(lr=(0.1, float("inf"))), "tensor 1: lr must be finite"),
    "lr nan": (_step, dict(lr=(float("nan"), 0.1)), "tensor 0: lr must be finite"),
    "null verdict": (_step, dict(verdict=0), "verdict is null"),
    "verdict at 2 mod 4": (_step, dict(verdict=0x4002), "verdict must be 4-byte"),
    "bf16 param at odd byte": (_step, dict(p=(0x1000, 0x1101)), "aligned"),
    "null param": (_step, dict(p=(0, 0x1100)), "null param"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_arguments_are_rejected(lib, case):
    from chocosgd_amd import _lib, codec
    call, kw, msg = BAD[case]
    before = codec.launch_count("sign_vote_kernel"), codec.launch_count("param_sign_step_kernel")
    assert call(lib, **kw) == ERR_INVALID, case
    err = _lib.last_error()
    assert msg in err, (case, err)
    assert (codec.launch_count("sign_vote_kernel"), codec.launch_count("param_sign_step_kernel")) == before


def test_no_words_launch_nothing(lib):
    from chocosgd_amd import codec
    before = codec.launch_count("sign_vote_kernel")
    assert _vote(lib, nwords=0) == 0 and codec.launch_count("sign_vote_kernel") == before


def test_launches_rule(lib):
    from chocosgd_amd import codec
    for nseg, want in [(-3, 0), (0, 0), (1, 1), (161, 1), (CAP, 1), (CAP + 1, 2), (2 * CAP + 3, 3)]:
        assert lib.choco_params_sign_step_launches(nseg) == want, nseg
        assert codec.params_sign_step_launches(nseg) == want
