"""signSGD / Signum with majority vote (Bernstein et al. 2019; the reference's `--majority_vote`
flag and SignCompressor.majority_vote, dl_code/pcode/utils/sparsification.py:165-181): every
worker sends the packed signs of its update direction, the ranks vote bit by bit, and the
parameters move by -lr times the voted sign.

`MajorityVoteCompressor(rank, world_size, aggregator, comm_device)`:
  * `.compress(flat)` -> sync_buffer with the packed signs of the flat fp32 buffer, no norms,
    written straight into the wire tensor (the batched sign pack);
  * `.sync(sync_buffer)` all-gathers ONE message of words per rank through a centralized
    aggregator (`_agg(..., communication_scheme="all_gather")`);
  * `.vote(sync_buffer)` -> the verdict over the gathered list in rank order
    (codec.sign_vote: packed to packed, one launch).

`fused_step(...)` is the step end to end: the batched apply_gradient in grad mode (d_p with
weight decay, momentum and Nesterov, written into the grads and a flat buffer), the sign pack,
sync, the vote, and ONE codec.params_sign_step launch (per chunk) that applies the packed verdict
to the parameter tensors.  Nothing is decoded to a dense buffer.  `step_loop(...)` is the same
step as one torch op per line (CPU tensors): the contract of the fused step.
"""
import torch

from . import codec, utils
from .communication import recover_device
from .sparsification import get_n_bits
from .tensor_buffer import TensorBuffer
from .wire import _staged


def step_loop(compressor, param_groups, param_names, state):
    """The majority-vote step as one torch op per line: the path CPU tensors, and anything the
    batched kernels do not take, keep.  The ranks exchange their dense +-1 tensors through the
    compressor's aggregator (all_gather, rank order).  NaN, +0 and -0 vote "+" (the pack's rule:
    bit set <=> d < 0); a tie is "+"."""
    entries = utils.step_entries(param_groups, param_names, "sign_sgd.step_loop", need_grads=True)
    utils.apply_gradient(param_groups, state, apply_grad_to_model=False)
    params = [p for _, p in entries]
    grads_tb = TensorBuffer([p.grad.data for p in params], dtype=torch.float32)
    s = torch.where(grads_tb.buffer < 0, -1.0, 1.0)
    gathered = compressor.aggregator_fn._agg(s, communication_scheme="all_gather", async_op=False)
    total = torch.stack([recover_device(t, device=s.device) for t in gathered]).sum(0)
    v = torch.where(total < 0, -1.0, 1.0)
    o = 0
    for group, p in entries:
        m = p.numel()
        p.data.add_(v[o:o + m].view_as(p.data).to(p.dtype), alpha=-group["lr"])
        o += m
    return 32 * (-(-o // 32))


def fused_step(compressor, param_groups, param_names, state, rounding=None, master=None, loss_scale=None,
               clip_norm=None):
    """One majority-vote signSGD step: utils.step_entries; the batched
    apply_gradient(apply_grad_to_model=False) writes d_p into the grads and a flat fp32 buffer in
    one launch per 72 tensors; the sign pack without norms; sync (one all_gather of the words); the
    vote on the packed words; ONE params_sign_step launch (per chunk) adds -lr * sign into the
    parameter tensors from the packed verdict, each tensor at its group's lr.  No unpack, no dense
    decode.  Returns n_bits, the nominal bits of one packed message.  Tensors the kernels do not
    take run step_loop.

    Not part of this step, each refused: rounding= (stochastic rounding),
    master= (fp32 master weights), loss_scale=, clip_norm=, and a weight decay decoupled from the
    voted sign (a group's "decoupled_weight_decay")."""
    what = "sign_sgd.fused_step"
    utils.no_rounding(what, rounding)
    for name, v in (("master", master), ("loss_scale", loss_scale), ("clip_norm", clip_norm)):
        if v is not None:
            raise RuntimeError(f"{what}: {name}= is not supported here -- the packed-sign update moves every "
                               "parameter by exactly lr, in the parameter's own dtype (DESIGN.md section 8)")
    if any(g.get("decoupled_weight_decay") for g in param_groups):
        raise RuntimeError(f"{what}: a weight decay decoupled from the voted sign is not supported -- weight_decay "
                           "enters d_p before the sign is taken, as apply_gradient has it")
    entries = utils.step_entries(param_groups, param_names, what, need_grads=True)
    first = entries[0][1]
    plan = flat = None
    if first.is_cuda:
        flat = torch.empty(sum(p.numel() for _, p in entries), dtype=torch.float32, device=first.device)
        plan = utils._sgd_fill(entries, state, False, flat)
    if plan is None:
        return step_loop(compressor, param_groups, param_names, state)
    plan.run(flat, grad_mode=True, write=True)
    sync_buffer = compressor.compress(flat)
    compressor.sync(sync_buffer)
    plan.sign_step(compressor.vote(sync_buffer))
    return sync_buffer["n_bits"]


class MajorityVoteCompressor(object):
    def __init__(self, rank, world_size, aggregator, comm_device, **kargs):
        if world_size > codec.MAX_VOTERS:
            raise RuntimeError(f"MajorityVoteCompressor: {world_size} voters, one vote takes {codec.MAX_VOTERS}; "
                               "hierarchical votes are not supported (a vote of partial votes is not the vote of all)")
        self.rank = rank
        self.world_size = world_size
        self.aggregator_fn = aggregator
        self.comm_device = comm_device
        self.kargs = kargs

    def compress(self, flat):
        words = torch.empty(codec.sign_words(flat.numel()), dtype=torch.int32, device=flat.device)
        codec.sign_compress(flat, want_norms=False, out=(words, None))  # written in place by the kernel
        return {"signs": words, "n_bits": get_n_bits(words)}

    def sync(self, sync_buffer):
        # the all-gather's list in rank order
        sync_buffer["synced_signs"] = list(self.aggregator_fn._agg(
            _staged(sync_buffer["signs"], self.comm_device), communication_scheme="all_gather", async_op=False))

    def vote(self, sync_buffer, weights=None):
        """The verdict of the gathered messages, on the device of this rank's own words."""
        if weights is not None:
            raise RuntimeError("MajorityVoteCompressor.vote: weighted votes are not supported (every voter counts "
                               "once; DESIGN.md section 8)")
        dev = sync_buffer["signs"].device
        return codec.sign_vote([recover_device(m, device=dev) for m in sync_buffer["synced_signs"]])
