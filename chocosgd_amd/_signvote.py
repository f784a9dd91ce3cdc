"""The Python side of the majority-vote entry points (csrc/vote.hip, csrc/signstep.hip).  codec.py
re-exports these as `codec.sign_vote`, `codec.params_sign_step`, `codec.params_sign_step_launches`
and `ParamSgdPlan.sign_step`; their stream-ordering cases stand in tests/test_gpu_sign_vote.py."""
import torch

from . import _lib
from . import codec as _c

MAX_VOTERS = 64  # voters of one sign_vote (vote.hip kVoteMax)


def sign_vote(messages, out=None):
    """The majority vote over packed sign words, packed to packed in one launch
    (include/choco_codec.h, choco_sign_vote): bit b of out[j] is set where strictly more than
    half of `messages` (1 to 64 int32 device tensors of one length) have it set; a tie gives 0,
    "+".  out (default: a new tensor) may be one of the messages.  Returns out."""
    messages = list(messages)
    if not 1 <= len(messages) <= MAX_VOTERS:
        raise RuntimeError(f"sign_vote takes 1 to {MAX_VOTERS} voters, got {len(messages)}: a vote of partial votes "
                           "is not the vote of all, so there is no chaining (DESIGN.md section 8)")
    named = [(f"message {q}", m) for q, m in enumerate(messages)]
    _c._require(messages[0], torch.int32, "message 0")
    dev, nwords = messages[0].device, messages[0].numel()
    if out is None:
        out = torch.empty(nwords, dtype=torch.int32, device=dev)
    else:
        named.append(("out", out))
    for name, t in named:
        _c._require(t, torch.int32, name)
        if t.numel() != nwords or t.device != dev:
            raise RuntimeError(f"{name} must hold {nwords} words on {dev}")
    ptrs, keep = _lib.ptr_array([m.data_ptr() for m in messages])
    _lib.check(_c.lib().choco_sign_vote(ptrs, len(messages), nwords, _c._ptr(out), _c._stream(dev)), "choco_sign_vote")
    return out


def plan_sign_step(plan, verdict):
    """ParamSgdPlan.sign_step: one choco_params_sign_step over the plan's tables as they stand."""
    _c._require(verdict, torch.int32, "verdict")
    if verdict.device != plan.device or verdict.numel() != _c.sign_words(plan.n):
        raise RuntimeError(f"verdict must hold {_c.sign_words(plan.n)} words on {plan.device}")
    _lib.check(_c.lib().choco_params_sign_step(plan.param_ptrs, plan.lens, plan.dts, plan.lr, plan.nseg,
                                               _c._ptr(verdict), plan.n, _c._stream(plan.device)),
               "choco_params_sign_step")


def params_sign_step_launches(nseg):
    """Launches one params_sign_step over `nseg` tensors takes."""
    return int(_c.lib().choco_params_sign_step_launches(int(nseg)))


def params_sign_step(params, verdict, lr, plan=None):
    """signSGD's update from a packed verdict, p.add_(sign, alpha=-lr) with one bit per element
    and no dense decode, one batched launch per chunk of tensors (include/choco_codec.h,
    choco_params_sign_step).  params: tensors laid out back to back in the flat space the verdict
    was packed from (sign_compress / sign_vote words, ceil(n / 32) of them); lr: a float or one
    per tensor.  Returns the plan (pass it back in to reuse its tables)."""
    params = list(params)
    if plan is None:
        plan = _c.ParamSgdPlan(params)
    elif not plan.holds(params):
        raise RuntimeError("the plan was built for another parameter list")
    for i, (p, a) in enumerate(zip(params, _c._per_tensor(lr, plan.nseg, "lr"))):
        if not p.is_contiguous():
            raise RuntimeError(f"param {i} must be contiguous")
        plan.param_ptrs[i], plan.lr[i] = p.data_ptr(), float(a)
    plan.seen = [None] * plan.nseg  # lr was written past the hyperparameter cache
    plan.sign_step(verdict)
    return plan
