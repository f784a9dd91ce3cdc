"""PowerGossip, host side (no GPU): powergossip.step_loop on a simulated ring against the exact gossip
step, DecentralizedAggregation.exchange_edges over gloo, and the C ABI's argument checks."""
import ctypes
import os
import threading

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_exchange_gloo import _free_port

KERNELS = ["lowrank_gossip_project_kernel", "lowrank_gossip_orth_kernel", "lowrank_gossip_backproject_kernel",
           "lowrank_gossip_slabsum_kernel", "lowrank_gossip_diff_kernel", "lowrank_gossip_apply_kernel"]
SHAPES = [(9, 11), (7,), (64, 147), (), (300, 9)]


class ThreadRing:
    """exchange_edges between worker threads of one process: a mailbox and a barrier."""
    box, bar = {}, None

    def __init__(self, rank):
        self.rank = rank

    def exchange_edges(self, messages):
        for j, t in messages.items():
            self.box[(self.rank, j)] = t
        self.bar.wait()
        got = {j: self.box[(j, self.rank)] for j in messages}
        self.bar.wait()
        return got


@pytest.mark.parametrize("r", [1, 2, 4])
def test_step_loop_is_the_exact_gossip_step_on_low_rank_differences(r):
    """X_i = base + a_i U V^T per matrix: every pairwise difference has rank r, so one power iteration
    recovers it and the step is X_i + sum_j w_ij (X_j - X_i).  The factors are large (|U V^T| ~ 1e3) so that
    the contract's 1e-8 in col / (||col|| + 1e-8) stays under the 1e-10 asked for: the step is off by
    2e-8 / ||dP col|| of the update, so it also takes a Q draw that is not nearly orthogonal to V (seed 0's are
    not; an edge whose draw has a cosine of 3e-4 to V, ||dP col|| = 5, shows the 1e-8 at 1.3e-9)."""
    from chocosgd_amd import powergossip
    from chocosgd_amd.communication import neighborhood
    rng, world = np.random.RandomState(r), 3
    base = [rng.standard_normal(s) for s in SHAPES]
    low = [30 * rng.standard_normal((s[0], r)) @ (30 * rng.standard_normal((r, int(np.prod(s[1:]))))) if len(s) > 1 else None
           for s in SHAPES]
    X0 = [[b + (i + 1) * (f.reshape(b.shape) if f is not None else rng.standard_normal(b.shape)) for b, f in zip(base, low)]
          for i in range(world)]
    models = [[torch.nn.Parameter(torch.from_numpy(np.asarray(x).copy())) for x in X0[i]] for i in range(world)]
    ThreadRing.box, ThreadRing.bar = {}, threading.Barrier(world)
    comps = [powergossip.PowerGossipCompressor(r, ThreadRing(i), neighborhood(i, world), seed=0) for i in range(world)]
    bits = [None] * world

    def run(i):
        groups = [{"params": [p], "name": f"p{k}", "lr": 0.1, "weight_decay": 0.0, "momentum": 0.0, "dampening": 0.0,
                   "nesterov": False} for k, p in enumerate(models[i])]  # no gradients: the local update is the identity
        bits[i] = powergossip.step_loop(comps[i], groups, list(enumerate(g["name"] for g in groups)), {})

    threads = [threading.Thread(target=run, args=(i,)) for i in range(world)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert bits[0] is not None and bits[0] == bits[1] == bits[2] and bits[0] > 0
    for k in range(len(SHAPES)):
        want = [X0[i][k] + sum((X0[j][k] - X0[i][k]) / 3 for j in range(world) if j != i) for i in range(world)]
        got = [models[i][k].detach().numpy() for i in range(world)]
        scale = max(np.abs(w).max() for w in want)
        assert all(np.abs(g - w).max() <= 1e-10 * scale for g, w in zip(got, want)), SHAPES[k]
        assert np.abs(sum(got) - sum(X0[i][k] for i in range(world))).max() <= 1e-10 * scale, "the mean is preserved"
    for i in range(world):  # both ends of an edge hold the same Q, bit for bit
        for e, j in enumerate(comps[i].neighbors):
            assert torch.equal(comps[i].q[e], comps[j].q[comps[j].neighbors.index(i)])


def _gloo_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from chocosgd_amd.communication import DecentralizedAggregation, neighborhood
        agg = DecentralizedAggregation(rank, neighborhood(rank, world))
        got = agg.exchange_edges({j: torch.full((5 + rank + j,), 10.0 * rank + j) for j in agg.neighbor_ranks})
        q.put((rank, {j: t.tolist() for j, t in got.items()}))
    finally:
        dist.destroy_process_group()


def test_exchange_edges_over_gloo():
    world, ctx = 3, mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, q)) for r in range(world)]
    [p.start() for p in procs]
    out = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank in range(world):
        others = [j for j in range(world) if j != rank]
        assert out[rank] == {j: [10.0 * j + rank] * (5 + rank + j) for j in others}, "what each neighbour addressed to it"


CALLS = {"project": "x q msg1 m1 m2", "orthogonalize": "msg1 recv1 m1 phat mask", "backproject": "x phat m1 msg2 m2 ws ws_bytes",
         "diff": "msg2 recv2 m1 m2 q dq mask", "apply": "x phat dq recv1 m1 m2 w mask"}
BAD = {"width 10": (dict(E=5), "n_edges * rank"), "no edges": (dict(E=0), "n_edges must be"),
       "short message 1": (dict(m1=5), "message 1"), "long message 2": (dict(m2=999), "message 2")}


@pytest.mark.parametrize("case,call", [(c, f) for c in sorted(BAD) for f in sorted(CALLS)
                                       if not (f == "orthogonalize" and "m2" in BAD[c][0])])  # it takes no message 2
def test_invalid_arguments_are_rejected(case, call):
    """The made-up device pointers are never dereferenced: every case is refused before the launch."""
    from chocosgd_amd import _lib, codec
    kw, msg = BAD[case]
    t = codec.LowRankPlan(SHAPES, 2, "cpu")
    a = dict(m1=t.msg1_len, m2=t.msg2_len, E=2, mask=1, ws_bytes=1 << 20, w=(ctypes.c_double * 8)(*[0.25] * 8))
    a.update({k: ctypes.c_void_p(0x1000 * (i + 1)) for i, k in enumerate("x q msg1 recv1 phat msg2 recv2 dq ws dev".split())})
    a.update(kw)
    before = [codec.launch_count(k) for k in KERNELS]
    fn = getattr(_lib.load(), "choco_lowrank_gossip_" + call)
    assert fn(*[a[k] for k in CALLS[call].split()], t.plan_host, a["dev"], t.n, 2, a["E"], None) < 0
    assert msg in _lib.last_error(), _lib.last_error()
    assert [codec.launch_count(k) for k in KERNELS] == before
    with pytest.raises(RuntimeError, match="n_edges"):
        codec.LowRankGossipPlan(SHAPES, 2, 5, "cpu")
