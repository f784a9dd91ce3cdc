"""The wide PowerGossip family, host side (no GPU): the C ABI's argument checks and codec.LowRankGossipWidePlan's range."""
import ctypes

import pytest

from test_powergossip_host import CALLS, SHAPES

KERNELS = ["lowrank_gossip_project_mfma_kernel", "lowrank_gossip_orth_kernel", "lowrank_gossip_backproject_mfma_kernel",
           "lowrank_gossip_slabsum_kernel", "lowrank_gossip_diff_kernel", "lowrank_gossip_apply_mfma_kernel"]
# the table's rank, what the call passes instead of a valid (rank 2, 5 edges) call, and what the message names
BAD = {"width 33 = 33 edges at rank 1": (1, dict(E=33), "n_edges * rank in (8, 32]"),
       "width 34": (2, dict(E=17), "n_edges * rank in (8, 32]"),
       "the narrow family's width": (2, dict(E=4), "n_edges * rank in (8, 32]"),
       "no edges": (2, dict(E=0), "n_edges must be at least 1"),
       "rank 3": (2, dict(rank=3), "rank must be 1, 2, 4, 8, 16 or 32"),
       "short message 1": (2, dict(m1=5), "message 1"), "long message 2": (2, dict(m2=999), "message 2")}


@pytest.mark.parametrize("case,call", [(c, f) for c in sorted(BAD) for f in sorted(CALLS)
                                       if not (f == "orthogonalize" and "m2" in BAD[c][1])])  # it takes no message 2
def test_invalid_arguments_are_rejected(case, call):
    """The made-up device pointers are never dereferenced: every case is refused before the launch."""
    from chocosgd_amd import _lib, codec
    r, kw, msg = BAD[case]
    t = codec.LowRankPlan(SHAPES, r, "cpu")
    a = dict(m1=t.msg1_len, m2=t.msg2_len, E=5, rank=r, mask=1, ws_bytes=1 << 20, w=(ctypes.c_double * 33)(*[0.25] * 33))
    a.update({k: ctypes.c_void_p(0x1000 * (i + 1)) for i, k in enumerate("x q msg1 recv1 phat msg2 recv2 dq ws dev".split())})
    a.update(kw)
    before = [codec.launch_count(k) for k in KERNELS]
    fn = getattr(_lib.load(), "choco_lowrank_gossip_wide_" + call)
    assert fn(*[a[k] for k in CALLS[call].split()], t.plan_host, a["dev"], t.n, a["rank"], a["E"], None) < 0
    assert msg in _lib.last_error(), _lib.last_error()
    assert [codec.launch_count(k) for k in KERNELS] == before


def test_plan_range():
    from chocosgd_amd import codec
    assert codec.GOSSIP_WIDE_MAX_WIDTH == 32
    with pytest.raises(RuntimeError, match="n_edges"):
        codec.LowRankGossipWidePlan(SHAPES, 2, 17, "cpu")
    wide, narrow = codec.LowRankGossipWidePlan(SHAPES, 4, 4, "cpu"), codec.LowRankGossipPlan(SHAPES, 4, 2, "cpu")
    assert (wide.n, wide.msg1_len, wide.msg2_len, wide.p_total) == (narrow.n, narrow.msg1_len, narrow.msg2_len, narrow.p_total)
    assert wide.ws_bytes >= 2 * (narrow.ws_bytes - 256) and wide.n_edges == 4
