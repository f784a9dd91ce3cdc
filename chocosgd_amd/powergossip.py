"""PowerGossip (Vogels, Karimireddy, Jaggi, "Practical low-rank communication compression in
decentralized deep learning", NeurIPS 2020): the low-rank compressor of powersgd.py on the gossip
path.  Every edge (i, j) of the graph runs a warm-started power iteration on X_i - X_j without either
end forming the difference: both ends multiply their own X by the edge's shared Q and swap the thin
products.  No error memory, no x_hat copies, no consensus step size.

`PowerGossipCompressor(rank, aggregator, neighbors_info, seed=0)` owns one worker's state.  The worker
is aggregator.rank = me; its neighbours j_0 < j_1 < .. < j_{E-1} are the keys of neighbors_info other
than me, w_e = neighbors_info[j_e], and edge e's low end is min(me, j_e).  Which tensors are compressed
is powersgd.is_compressed(shape, rank).  Per edge and compressed tensor there is a Q_e (cols x r), drawn
with torch.randn from a CPU generator seeded by (seed, min(me, j_e), max(me, j_e)), in layout order:
both ends of an edge start from the same Q_e.

One step (X: the flat buffer of the parameters after the local update):
  1. local update   apply_gradient fused with the pack of the new parameters into X
  2. project        P_e = X Q_e per edge; message 1 of edge e = [P_e,0 | P_e,1 | .. | the uncompressed
                    tensors of X] (codec.LowRankPlan's message-1 layout)
  3. exchange message 1 per edge (aggregator.exchange_edges)
  4. orthogonalise  dP_e = P(lo end) - P(hi end), in that operand order at both ends; P^_e = modified
                    Gram-Schmidt of dP_e (powersgd.orthogonalize_loop)
  5. back-project   Q'_e = X^T P^_e; message 2 of edge e = [Q'_e,0 | ..]
  6. exchange message 2 per edge
  7. difference     dQ_e = Q'(lo end) - Q'(hi end) becomes the edge's next Q_e -- except a matrix whose
                    dQ_e is zero in every element, which keeps its Q_e (an edge that once agrees exactly
                    would otherwise be dead for good)
  8. apply          compressed: X += sum_e c_e P^_e dQ_e^T, edges ascending, c_e = -w_e at the low end and
                    +w_e at the high end;  uncompressed: x += sum_e w_e (x_received,e - x);  then unpack

Steps 4 and 7 see the same two operands in the same order at both ends, so P^_e, dQ_e and the stored Q_e
are bit-identical at the two ends of an edge and the two updates are each other's negation up to the
final add.  `fused_step(...)` runs the step as batched launches, each of which passes over X once for ALL
edges: codec.LowRankGossipPlan's (csrc/lowrank_gossip.hip) where E * rank <= 8 at rank <= 4, else
codec.LowRankGossipWidePlan's on the fp32 matrix instruction (csrc/lowrank_gossip_mfma.hip) where E * rank <= 32;
`step_loop(...)` is the same step as one torch op per line, in the tensors' own precision (fp64 models stay
fp64): the readable contract, and the path for CPU tensors, E * rank > 32 and anything the batched kernels do
not take.
"""
import torch

from . import codec, powersgd, utils


class PowerGossipCompressor(object):
    def __init__(self, rank, aggregator, neighbors_info, seed=0):
        if rank not in codec.LOWRANK_RANKS:
            raise RuntimeError(f"PowerGossipCompressor: rank must be one of {codec.LOWRANK_RANKS}, got {rank} "
                               "(DESIGN.md section 8)")
        self.rank, self.aggregator_fn, self.neighbors_info, self.seed = rank, aggregator, neighbors_info, seed
        self.me = aggregator.rank
        self.neighbors = sorted(j for j in neighbors_info if j != self.me)
        self.weights = [float(neighbors_info[j]) for j in self.neighbors]
        self.lo = [self.me < j for j in self.neighbors]
        self.lo_mask = sum(1 << e for e, low in enumerate(self.lo) if low)
        self.shapes = self.q = self.plan = None

    def state(self, shapes, device, dtype=torch.float32):
        """The worker's state for this layout, created on first use: .q, (E, msg2_len), row e = [Q_e,0 |
        Q_e,1 | ..], and, on a ROCm device in fp32, .plan: codec.LowRankGossipPlan where it applies (E * rank <= 8
        at rank <= 4), else codec.LowRankGossipWidePlan where E * rank <= 32, else None.  Another layout, device
        or dtype later on raises."""
        shapes = [tuple(int(d) for d in s) for s in shapes]
        if self.shapes is None:
            rows = []
            for j in self.neighbors:
                lo, hi = min(self.me, j), max(self.me, j)
                gen = torch.Generator().manual_seed((int(self.seed) * 1000003 + lo) * 1000003 + hi)
                rows.append(torch.cat([torch.randn(torch.Size(s).numel() // s[0], self.rank, generator=gen).reshape(-1)
                                       for s in shapes if powersgd.is_compressed(s, self.rank)] + [torch.empty(0)]))
            self.q = torch.stack(rows).to(device=device, dtype=dtype) if rows else torch.empty(0, 0, device=device, dtype=dtype)
            cls = plan_class(self.rank, len(self.neighbors))
            if self.q.is_cuda and dtype == torch.float32 and cls is not None:
                self.plan = cls(shapes, self.rank, len(self.neighbors), device)
            self.shapes = shapes
        elif shapes != self.shapes or self.q.device != torch.device(device) or self.q.dtype != dtype:
            raise RuntimeError("PowerGossipCompressor: the edges' Q were created for another layout "
                               f"({len(self.shapes)} tensors on {self.q.device}, {self.q.dtype}); use one compressor "
                               "per model")
        return self


def plan_class(rank, n_edges):
    """The batched kernel family of a worker with n_edges edges at this rank: the narrow plan where it applies,
    the wide plan where E * rank <= 32, None (step_loop) otherwise."""
    width = n_edges * rank
    if 1 <= width <= codec.GOSSIP_MAX_WIDTH and rank <= 4:
        return codec.LowRankGossipPlan
    if 1 <= width <= codec.GOSSIP_WIDE_MAX_WIDTH:
        return codec.LowRankGossipWidePlan
    return None


def step_loop(compressor, param_groups, param_names, state):
    """The PowerGossip step as one torch op per line, tensor and edge.  Returns n_bits of the 2 E messages."""
    entries = utils.step_entries(param_groups, param_names, "powergossip.step_loop")
    params = [p for _, p in entries]
    dt = torch.float64 if all(p.dtype == torch.float64 for p in params) else torch.float32
    r, agg, nbrs = compressor.rank, compressor.aggregator_fn, compressor.neighbors
    st = compressor.state([p.shape for p in params], params[0].device, dt)
    # 1. the local update
    utils.apply_gradient_loop(param_groups, state, True)
    X = [p.data.reshape(p.shape[0], -1).to(dt) if powersgd.is_compressed(p.shape, r) else p.data.reshape(-1).to(dt)
         for p in params]
    mats = [x for x in X if x.dim() == 2]
    rest = [x for x in X if x.dim() == 1]
    q_off = [sum(m.shape[1] * r for m in mats[:k]) for k in range(len(mats))]
    p_off = [sum(m.shape[0] * r for m in mats[:k]) for k in range(len(mats) + 1)]
    empty = torch.empty(0, dtype=dt, device=params[0].device)

    def Q(src, k):
        return src[q_off[k]:q_off[k] + mats[k].shape[1] * r].view(mats[k].shape[1], r)

    # 2. project, 3. exchange
    msg1 = {j: torch.cat([(m @ Q(st.q[e], k)).reshape(-1) for k, m in enumerate(mats)] + rest + [empty])
            for e, j in enumerate(nbrs)}
    recv1 = agg.exchange_edges(msg1)
    # 4. difference (lo end - hi end) and orthogonalise, 5. back-project, 6. exchange
    Ph = []
    for j, low in zip(nbrs, compressor.lo):
        dP = msg1[j] - recv1[j] if low else recv1[j] - msg1[j]
        Ph.append([powersgd.orthogonalize_loop(dP[p_off[k]:p_off[k + 1]].view(m.shape[0], r).clone())
                   for k, m in enumerate(mats)])
    msg2 = {j: torch.cat([(m.t() @ Ph[e][k]).reshape(-1) for k, m in enumerate(mats)] + [empty]) for e, j in enumerate(nbrs)}
    recv2 = agg.exchange_edges(msg2)
    # 7. difference; the edge's next Q unless it is all zeros
    dQ = [msg2[j] - recv2[j] if low else recv2[j] - msg2[j] for j, low in zip(nbrs, compressor.lo)]
    for e in range(len(nbrs)):
        for k in range(len(mats)):
            if Q(dQ[e], k).ne(0).any():
                Q(st.q[e], k).copy_(Q(dQ[e], k))
    # 8. apply, unpack
    signed = [-w if low else w for w, low in zip(compressor.weights, compressor.lo)]
    k = t = 0
    for p, x in zip(params, X):
        if not nbrs:
            break
        if x.dim() == 2:
            upd = signed[0] * (Ph[0][k] @ Q(dQ[0], k).t())
            for e in range(1, len(nbrs)):
                upd = upd + signed[e] * (Ph[e][k] @ Q(dQ[e], k).t())
            k += 1
        else:
            at = p_off[-1] + t
            upd = compressor.weights[0] * (recv1[nbrs[0]][at:at + x.numel()] - x)
            for e in range(1, len(nbrs)):
                upd = upd + compressor.weights[e] * (recv1[nbrs[e]][at:at + x.numel()] - x)
            t += x.numel()
        p.data.copy_((x + upd).reshape(p.shape))
    return 32 * len(nbrs) * (p_off[-1] + sum(x.numel() for x in rest) + sum(m.shape[1] * r for m in mats))


def fused_step(compressor, param_groups, param_names, state, master=None, clip_norm=None, loss_scale=None, rounding=None):
    """One PowerGossip step end to end: utils.step_entries, apply_gradient fused with the pack of the new
    parameters into flat X (as utils.dpsgd_step starts; the parameters are not written yet),
    lowrank_gossip_project_kernel, the exchange of message 1, lowrank_gossip_orth_kernel,
    lowrank_gossip_backproject_kernel (and the slab-sum launch), the exchange of message 2,
    lowrank_gossip_diff_kernel, lowrank_gossip_apply_kernel and the batched unpack of X into the parameters.
    Beyond E * rank = 8 or rank 4, up to E * rank = 32, project, back-project and apply are
    lowrank_gossip_{project,backproject,apply}_mfma_kernel (plan_class).  Every kernel that touches X passes
    over it once for all E edges.  Returns n_bits = 32 E (msg1_len + msg2_len).  Tensors the kernels do not
    take, no neighbours, or E * rank > 32 run step_loop.

    Not part of this step, each refused: master=, clip_norm=, loss_scale= and
    rounding=."""
    what = "powergossip.fused_step"
    utils.no_rounding(what, rounding)
    for name, v in (("master", master), ("clip_norm", clip_norm), ("loss_scale", loss_scale)):
        if v is not None:
            raise RuntimeError(f"{what}: {name}= is not supported here -- the step exchanges projections of the plain "
                               "fp32 update of the parameters (DESIGN.md section 8)")
    entries = utils.step_entries(param_groups, param_names, what)
    params = [p for _, p in entries]
    nbrs, E = compressor.neighbors, len(compressor.neighbors)
    if plan_class(compressor.rank, E) is None or not params[0].is_cuda:
        return step_loop(compressor, param_groups, param_names, state)
    flat = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=params[0].device)
    plan = utils._sgd_fill(entries, state, True, flat)
    if plan is None:
        return step_loop(compressor, param_groups, param_names, state)
    st = compressor.state([p.shape for p in params], plan.device)
    gp, agg = st.plan, compressor.aggregator_fn
    plan.run(flat, grad_mode=False, write=False)

    def exchange(own, per_edge):
        got = torch.empty_like(own)
        agg.exchange_edges({j: own.view(E, per_edge)[e] for e, j in enumerate(nbrs)},
                           out={j: got.view(E, per_edge)[e] for e, j in enumerate(nbrs)})
        return got

    msg1 = torch.empty(E * gp.msg1_len, dtype=torch.float32, device=plan.device)
    gp.project(flat, st.q.view(-1), msg1)
    recv1 = exchange(msg1, gp.msg1_len)
    phat = torch.empty(E * gp.p_total, dtype=torch.float32, device=plan.device)
    gp.orthogonalize(msg1, recv1, phat, compressor.lo_mask)
    msg2 = torch.empty(E * gp.msg2_len, dtype=torch.float32, device=plan.device)
    gp.backproject(flat, phat, msg2)
    recv2 = exchange(msg2, gp.msg2_len)
    dq = torch.empty_like(msg2)
    gp.diff(msg2, recv2, st.q.view(-1), dq, compressor.lo_mask)
    gp.apply(flat, phat, dq, recv1, compressor.weights, compressor.lo_mask)
    codec.params_unpack(flat, [p.data for p in params])
    return 32 * E * (gp.msg1_len + gp.msg2_len)
