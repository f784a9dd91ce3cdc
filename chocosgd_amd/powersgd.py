"""Rank-r PowerSGD (Vogels, Karimireddy, Jaggi, NeurIPS 2019) with error feedback on the
all-reduce path: the one compressor of this family whose messages can be SUMMED, so it rides
`CentralizedAggregation._agg(op="sum")` twice per step instead of an all-gather.

A tensor of at least two dimensions with rows * cols > r * (rows + cols) (rows = shape[0], cols
= numel / rows) is compressed: it is the row-major matrix M (rows x cols) of the flat gradient
buffer.  Every other tensor -- vectors, scalars, empty tensors, matrices too small to save
anything -- travels as it is.  `PowerSGDCompressor(rank, aggregator, seed=0, orthogonalize="mgs")` owns the state of one
worker: the flat error memory `e` (zero at first) and, per compressed tensor, `Q` (cols x r), drawn
with torch.randn from a CPU generator seeded with `seed`, in layout order, so every rank starts
from the same Q.

One step (g: the flat fp32 gradient; W: the divisor, the world size):
  1. project        M = g + e (kept in place of e), P = M Q;  message 1 = [P_0 | P_1 | .. | the
                    uncompressed tensors' gradients]
  2. all-reduce (sum) message 1
  3. orthogonalise  modified Gram-Schmidt on the columns of every summed P, in column order:
                    col /= (||col|| + 1e-8), later -= (col . later) col
                    (orthogonalize="cholqr", ranks 8, 16 and 32: the same P^ by Cholesky-QR --
                    G = P^T P in fp64, G = L L^T with a pivot rule, P^ = P L^-T D, one rounding;
                    `orthogonalize_cholqr_loop`)
  4. back-project   Q = M^T P^;  message 2 = [Q_0 | Q_1 | ..]
  5. all-reduce (sum) message 2; the summed Q is what the next step starts from (step 3
     normalises, so it is not divided)
  6. decode         compressed: sum = P^ Q^T, e = M - sum / W;  uncompressed: sum = the tail
  7. the plain SGD update from the flat summed gradient (ParamSgdPlan.run_flatgrad, unchanged)

`fused_step(...)` runs it as codec.LowRankPlan's four launches (csrc/lowrank.hip at rank 1, 2 and
4; csrc/lowrank_mfma.hip's matrix-instruction kernels at rank 8, 16 and 32) between the gradient
pack and the flat-gradient update.  Any other rank raises.  `step_loop(...)` is the same step as one torch op
per line and tensor, in the tensors' own precision (fp64 models stay fp64): the readable
contract, and the path for CPU tensors and anything the batched kernels do not take.
"""
import torch

from . import codec, utils

EPS = 1e-8


def is_compressed(shape, rank):
    """Whether a tensor of `shape` travels as rank-`rank` factors."""
    shape = tuple(shape)
    numel = 1
    for d in shape:
        numel *= int(d)
    if len(shape) < 2 or numel == 0:
        return False
    rows, cols = int(shape[0]), numel // int(shape[0])
    return rows * cols > rank * (rows + cols)


class PowerSGDCompressor(object):
    def __init__(self, rank, aggregator, seed=0, orthogonalize="mgs"):
        if rank not in codec.LOWRANK_RANKS:
            raise RuntimeError(f"PowerSGDCompressor: rank must be one of {codec.LOWRANK_RANKS}, got {rank} "
                               "(DESIGN.md section 8)")
        if orthogonalize not in codec.LOWRANK_ORTH_METHODS:
            raise RuntimeError(f"PowerSGDCompressor: orthogonalize must be one of {codec.LOWRANK_ORTH_METHODS}, got "
                               f"{orthogonalize!r}")
        if orthogonalize == "cholqr" and rank < 8:
            raise RuntimeError(f"PowerSGDCompressor: orthogonalize=\"cholqr\" is built for ranks 8, 16 and 32, got {rank}; "
                               "ranks 1, 2 and 4 keep modified Gram-Schmidt (DESIGN.md section 8)")
        self.rank, self.aggregator_fn, self.seed, self.orthogonalize = rank, aggregator, seed, orthogonalize
        self.shapes = self.e = self.q = self.plan = None

    def state(self, shapes, device, dtype=torch.float32):
        """The worker's state for this layout, created on first use: .e (flat, zero), .q
        ([Q_0 | Q_1 | ..], flat) and, on a ROCm device in fp32, .plan (codec.LowRankPlan).
        Another layout, device or dtype later on raises."""
        shapes = [tuple(int(d) for d in s) for s in shapes]
        if self.shapes is None:
            gen = torch.Generator().manual_seed(self.seed)
            qs = [torch.randn(torch.Size(s).numel() // s[0], self.rank, generator=gen).reshape(-1)
                  for s in shapes if is_compressed(s, self.rank)]
            self.q = torch.cat(qs + [torch.empty(0)]).to(device=device, dtype=dtype)
            self.e = torch.zeros(sum(torch.Size(s).numel() for s in shapes), device=device, dtype=dtype)
            if self.e.is_cuda and dtype == torch.float32:
                self.plan = codec.LowRankPlan(shapes, self.rank, device)
            self.shapes = shapes
        elif shapes != self.shapes or self.e.device != torch.device(device) or self.e.dtype != dtype:
            raise RuntimeError("PowerSGDCompressor: the error memory and Q were created for another layout "
                               f"({len(self.shapes)} tensors on {self.e.device}, {self.e.dtype}); use one compressor "
                               "per model")
        return self


def orthogonalize_loop(P):
    """Modified Gram-Schmidt in place on the columns of P, in column order."""
    for k in range(P.shape[1]):
        col = P[:, k]
        col /= col.norm() + EPS
        for j in range(k + 1, P.shape[1]):
            P[:, j] -= (col @ P[:, j]) * col
    return P


TAU = 2.0 ** -30  # a Cholesky pivot at or under TAU G_kk drops its column


def orthogonalize_cholqr_loop(P):
    """Cholesky-QR in place on the columns of P: the P^ of orthogonalize_loop (the thin QR factorisation
    with a positive diagonal is unique) from an fp64 Gram matrix, whatever P's dtype, and one cast."""
    P64, r = P.double(), P.shape[1]
    G = P64.t() @ P64
    L = torch.zeros_like(G)
    for k in range(r):
        d = G[k, k] - (L[k, :k] * L[k, :k]).sum()
        if d <= TAU * G[k, k]:  # nothing new in this column (a zero column too): dropped
            continue
        L[k, k] = d.sqrt()
        L[k + 1:, k] = (G[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
    keep = (L.diagonal() > 0).nonzero().reshape(-1)
    T = torch.zeros_like(G)  # T = L^-T D over the kept columns, D_kk = L_kk / (L_kk + EPS): Gram-Schmidt's divisor
    T[keep[:, None], keep] = torch.linalg.inv(L[keep][:, keep]).t() * (L.diagonal() / (L.diagonal() + EPS))[keep]
    P.copy_((P64 @ T).to(P.dtype))
    return P


def step_loop(compressor, param_groups, param_names, state, distributed=True, write_grads=True):
    """The PowerSGD step as one torch op per line and tensor.  Returns n_bits of the two messages."""
    entries = utils.step_entries(param_groups, param_names, "powersgd.step_loop", need_grads=True)
    grads = [p.grad.data for _, p in entries]
    dt = torch.float64 if all(g.dtype == torch.float64 for g in grads) else torch.float32
    st = compressor.state([g.shape for g in grads], grads[0].device, dt)
    r, agg = compressor.rank, compressor.aggregator_fn
    comp = [is_compressed(g.shape, r) for g in grads]
    sizes = [g.numel() for g in grads]
    offs = [sum(sizes[:t]) for t in range(len(sizes))]
    # 1. project
    Ms, Ps, qo, q_offs = [], [], 0, []
    for g, c, o in zip(grads, comp, offs):
        if not c:
            continue
        rows, cols = g.shape[0], g.numel() // g.shape[0]
        M = g.reshape(rows, cols).to(dt) + st.e[o:o + g.numel()].view(rows, cols)
        st.e[o:o + g.numel()] = M.reshape(-1)
        Ms.append(M)
        Ps.append(M @ st.q[qo:qo + cols * r].view(cols, r))
        q_offs.append(qo)
        qo += cols * r
    msg1 = torch.cat([P.reshape(-1) for P in Ps] + [g.reshape(-1).to(dt) for g, c in zip(grads, comp) if not c])
    # 2. all-reduce
    msg1 = agg._agg(msg1, op="sum", distributed=distributed)
    # 3. orthogonalise, 4. back-project
    po, Phs, Qs = 0, [], []
    orth = orthogonalize_cholqr_loop if compressor.orthogonalize == "cholqr" else orthogonalize_loop
    for M in Ms:
        Phs.append(orth(msg1[po:po + M.shape[0] * r].view(M.shape[0], r).clone()))
        Qs.append(M.t() @ Phs[-1])
        po += M.shape[0] * r
    msg2 = torch.cat([Q.reshape(-1) for Q in Qs] + [torch.empty(0, dtype=dt, device=msg1.device)])
    # 5. all-reduce; the summed Q starts the next step
    msg2 = agg._agg(msg2, op="sum", distributed=distributed)
    st.q = msg2
    # 6. decode
    divisor = torch.full((), float(agg.world_size) if distributed else 1.0, dtype=dt, device=msg1.device)
    avg, k = [], 0
    for g, c, o in zip(grads, comp, offs):
        if c:
            total = Phs[k] @ msg2[q_offs[k]:q_offs[k] + Qs[k].numel()].view_as(Qs[k]).t()
            avg.append((total / divisor).reshape(g.shape))
            st.e[o:o + g.numel()] = (Ms[k] - avg[-1].view_as(Ms[k])).reshape(-1)
            k += 1
        else:
            avg.append((msg1[po:po + g.numel()] / divisor).reshape(g.shape))
            po += g.numel()
    # 7. the update on the averaged gradient
    if dt == torch.float64:  # apply_gradient_loop's lines in the model's own precision
        saved = None if write_grads else [g.clone() for g in grads]
        for g, a in zip(grads, avg):
            g.copy_(a)
        utils.apply_gradient_loop(param_groups, state)
        for g, s in zip(grads, saved or []):
            g.copy_(s)
    else:
        narrowed = [a.to(g.dtype) for a, g in zip(avg, grads)]
        if write_grads:
            for g, a in zip(grads, narrowed):
                g.copy_(a)
        utils._apply_averaged_loop(entries, state, narrowed)
    return 32 * (msg1.numel() + msg2.numel())


def fused_step(compressor, param_groups, param_names, state, distributed=True, write_grads=True, master=None,
               clip_norm=None, loss_scale=None, rounding=None):
    """One PowerSGD step end to end: utils.step_entries, ONE pack launch per chunk of the
    gradients into a flat fp32 buffer (16-bit gradients are widened), lowrank_project_kernel,
    the all-reduce of message 1, lowrank_orth_kernel (the compressor's orthogonalize="cholqr":
    lowrank_gram_kernel, lowrank_chol_kernel, lowrank_orthapply_kernel), lowrank_backproject_kernel (and the
    slab-sum launch), the all-reduce of message 2, lowrank_decode_kernel (at rank 8, 16 and 32
    the lowrank_*_mfma_kernel of project, back-project and decode), and the flat-gradient
    SGD update (ParamSgdPlan.run_flatgrad, which divides by the same divisor and narrows).
    Returns n_bits = 32 * (msg1_len + msg2_len).  write_grads: p.grad receives the decoded
    average.  Tensors the kernels do not take run step_loop.

    Not part of this step, each refused: master=, clip_norm=, loss_scale=
    and rounding=.  For a 16-bit model the narrowing loss of the update is not fed back into
    the error memory."""
    what = "powersgd.fused_step"
    utils.no_rounding(what, rounding)
    for name, v in (("master", master), ("clip_norm", clip_norm), ("loss_scale", loss_scale)):
        if v is not None:
            raise RuntimeError(f"{what}: {name}= is not supported here -- the error memory is taken against the plain "
                               "fp32 average of the decoded gradients (DESIGN.md section 8)")
    entries = utils.step_entries(param_groups, param_names, what, need_grads=True)
    plan = utils._sgd_fill(entries, state, True, None)
    if plan is None:
        return step_loop(compressor, param_groups, param_names, state, distributed, write_grads)
    st = compressor.state([p.shape for _, p in entries], plan.device)
    lr, agg = st.plan, compressor.aggregator_fn
    flat = torch.empty(plan.n, dtype=torch.float32, device=plan.device)
    plan.pack_grads(flat)
    msg1 = torch.empty(lr.msg1_len, dtype=torch.float32, device=plan.device)
    lr.project(flat, st.e, st.q, msg1)
    msg1 = agg._agg(msg1, op="sum", distributed=distributed)
    lr.orthogonalize(msg1, compressor.orthogonalize)
    msg2 = torch.empty(lr.msg2_len, dtype=torch.float32, device=plan.device)
    lr.backproject(st.e, msg1, msg2)
    msg2 = st.q = agg._agg(msg2, op="sum", distributed=distributed)
    divisor = float(agg.world_size) if distributed else 1.0
    lr.decode(st.e, msg1, msg2, flat, divisor)  # the gradient buffer has been consumed: it takes the sum
    plan.run_flatgrad(flat, divisor, write=True, write_grads=write_grads)
    return 32 * (lr.msg1_len + lr.msg2_len)
