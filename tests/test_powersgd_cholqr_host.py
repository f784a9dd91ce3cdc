"""Cholesky-QR orthogonalisation, host side (no GPU): the entry point's refusals (each before any launch), the
compressor's, and powersgd.orthogonalize_cholqr_loop against the numpy oracle of the contract."""
import ctypes

import numpy as np
import pytest
import torch

import _cholqr_oracle as CO

KERNELS = ["lowrank_gram_kernel", "lowrank_chol_kernel", "lowrank_orthapply_kernel"]
BAD = {"rank 4": (4, {}, "built for ranks 8, 16 and 32"), "null workspace": (8, dict(ws=0), "null workspace"),
       "short workspace": (8, dict(ws_bytes=64), "workspace too small"), "null msg1": (8, dict(msg1=0), "null msg1"),
       "another table's rank": (8, dict(rank=16), "built for rank")}


@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_arguments_are_rejected(case):
    """The made-up device pointers are never dereferenced: every case is refused before the launch."""
    from chocosgd_amd import _lib, codec
    r, kw, msg = BAD[case]
    plan = codec.LowRankPlan([(300, 40), (7,), (64, 80)], r, "cpu")
    assert (plan.orth_ws_bytes > 0) == (r >= 8)
    a = dict(dict(msg1=0x4000, ws=0x7000, ws_bytes=1 << 20, rank=r), **kw)
    before = [codec.launch_count(k) for k in KERNELS]
    rc = _lib.load().choco_lowrank_orthogonalize_cholqr(ctypes.c_void_p(a["msg1"]), plan.msg1_len, ctypes.c_void_p(a["ws"]), a["ws_bytes"],
                                                        plan.plan_host, ctypes.c_void_p(0x8000), plan.n, a["rank"], None)
    assert rc == -1 and msg in _lib.last_error(), _lib.last_error()
    assert [codec.launch_count(k) for k in KERNELS] == before
    from chocosgd_amd import powersgd
    with pytest.raises(RuntimeError, match="DESIGN.md section 8"):
        powersgd.PowerSGDCompressor(4, None, orthogonalize="cholqr")
    with pytest.raises(RuntimeError, match="orthogonalize must be"):
        powersgd.PowerSGDCompressor(8, None, orthogonalize="householder")


@pytest.mark.parametrize("r,rows", [(8, 12), (16, 257), (32, 600)])
def test_loop_matches_the_oracle(r, rows):
    """fp64 P with a zero and a duplicated column; both sides fp64, apart by the Gram's summation order and L's inversion:
    at most rows 2^-53 x the condition number squared (under 40 here) of elements under 1, 2e-13; 1e-11 leaves a factor 50."""
    from chocosgd_amd import powersgd
    P = np.random.RandomState(r).standard_normal((rows, r))
    P[:, 2], P[:, 5] = 0.0, P[:, 1]
    want = CO.orthogonalize(P)
    assert not want[:, 2].any() and not want[:, 5].any() and np.abs(want[:, r - 1]).max() > 0.01
    np.testing.assert_allclose(powersgd.orthogonalize_cholqr_loop(torch.from_numpy(P.copy())).numpy(), want, rtol=0, atol=1e-11)
