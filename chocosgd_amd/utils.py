"""Optimizer-step helpers: drop-in for dl_code/pcode/optim/utils.py (apply_gradient and the
CHOCO half)."""
import torch

from . import codec
from .rounding import StochasticRounding, sr_bits, sr_narrow_bf16, sr_pair  # noqa: F401  (re-exported)
from .sparsification import get_n_bits
from .tensor_buffer import TensorBuffer, flatten


def _get_data(param_groups, idx, is_get_grad):
    if is_get_grad:
        return param_groups[idx]["params"][0].grad
    return param_groups[idx]["params"][0]


def apply_gradient_loop(param_groups, state, apply_grad_to_model=True):
    """apply_gradient as one torch op per line and tensor (optim/utils.py:13-47): the path CPU
    tensors, and anything the batched kernel does not take, keep.  Same results as the
    reference, with the two differences apply_gradient documents."""
    for group in param_groups:
        weight_decay, momentum = group["weight_decay"], group["momentum"]
        dampening, nesterov = group["dampening"], group["nesterov"]
        for p in group["params"]:
            if p.grad is None:
                continue
            d_p = p.grad.data
            if weight_decay != 0:
                d_p = d_p.add(p.data, alpha=weight_decay)  # out of place: p.grad keeps its values
            if momentum != 0:
                param_state = state[p]
                if "momentum_buffer" not in param_state:
                    buf = param_state["momentum_buffer"] = torch.zeros_like(p.data)
                    buf.mul_(momentum).add_(d_p)
                else:
                    buf = param_state["momentum_buffer"]
                    buf.mul_(momentum).add_(d_p, alpha=1 - dampening)
                d_p = d_p.add(buf, alpha=momentum) if nesterov else buf
            if apply_grad_to_model:
                p.data.add_(d_p, alpha=-group["lr"])
            else:
                p.grad.data.copy_(d_p)  # into the grad's own storage: p.grad is not rebound


def _params_with_grad(parameters):
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    return [p for p in parameters if p.grad is not None]


def _total_norm(grads, total_norm, coef_dtype):
    """The total L2 norm of `grads` as a 0-dim tensor of coef_dtype: sqrt of the fp64 sum of
    squares over every element, rounded once to fp32 and then to coef_dtype -- or `total_norm`
    (a tensor or a float) in its place."""
    dev = grads[0].device
    if total_norm is not None:
        return torch.as_tensor(total_norm, dtype=torch.float32).detach().reshape(()).to(dev).to(coef_dtype)
    sq = [g.detach().double().pow(2).sum().to(dev) for g in grads]
    return torch.stack(sq).sum().sqrt().float().to(coef_dtype)


def clip_grad_norm_loop(parameters, max_norm, total_norm=None, norm_type=2.0):
    """torch.nn.utils.clip_grad_norm_ (distributed_running_nlp.py:96) with torch ops: the path
    CPU tensors, and anything the batched kernels do not take, keep.  The total is this
    package's (_total_norm: fp64 accumulation, one rounding to fp32 and one to the gradients'
    common dtype) unless one is given; the scaling is torch.nn.utils.clip_grads_with_norm_.
    norm_type != 2: torch's own total (torch.nn.utils.get_total_norm).  Returns the total."""
    params = _params_with_grad(parameters)
    if not params:
        return torch.tensor(0.0)
    grads = [p.grad for p in params]
    if float(norm_type) != 2.0 and total_norm is None:
        total = torch.nn.utils.get_total_norm(grads, norm_type)
    else:
        total = _total_norm(grads, total_norm, codec.common_grad_dtype(g.dtype for g in grads))
    torch.nn.utils.clip_grads_with_norm_(params, max_norm, total)
    return total


def _clip_plan(params):
    """The plan of `params` (each with a gradient) filled for the clip alone: grad mode, zero
    hyperparameter tables, no buffers; None where a tensor cannot take the batched kernels."""
    plan = _sgd_plan(params)
    if plan is None or not all(plan.fits(i, p.grad) for i, p in enumerate(params)):
        return None
    zero = (0.0, 0.0, 0.0, 0.0)
    for i, p in enumerate(params):
        plan.param_ptrs[i], plan.grad_ptrs[i], plan.buf_ptrs[i], plan.flags[i] = p.data_ptr(), p.grad.data_ptr(), None, 0
        if plan.seen[i] != zero:
            plan.lr[i], plan.weight_decay[i], plan.momentum[i], plan.dampening[i] = zero
            plan.seen[i] = zero
    return plan


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None, total_norm=None):
    """Drop-in for torch.nn.utils.clip_grad_norm_(model.parameters(), conf.rnn_clip)
    (distributed_running_nlp.py:96): scales the gradients in place by
    min(1, max_norm / (total + 1e-6)), torch's own op sequence for the coefficient, and returns
    the total norm as a 0-dim device tensor (a copy).  fp32 / bf16 / fp16 ROCm gradients take
    one norm pass (codec ParamSgdPlan.gradnorm) and ONE launch per chunk of tensors that reads
    each gradient once and writes it once; the coefficient never leaves the device.  Parameters
    without a gradient are skipped.  CPU tensors, other dtypes, non-contiguous gradients,
    several devices and norm_type != 2 take clip_grad_norm_loop.

    One difference from torch, by design: the total is sqrt of the fp64 sum of squares over all
    elements, rounded once to fp32 (and to a 16-bit common dtype), not the norm of per-tensor
    fp32 norms.  total_norm (a tensor or a float) pins the total instead.  `foreach` is
    accepted and ignored.  error_if_nonfinite reads the total on the host, the only case that
    does."""
    params = _params_with_grad(parameters)
    plan = _clip_plan(params) if params and float(norm_type) == 2.0 else None
    if plan is None:
        total = clip_grad_norm_loop(params, max_norm, total_norm, norm_type)
    else:
        out = plan.gradnorm(max_norm, total_norm=total_norm)
        plan.run(None, grad_mode=True, write=True, gclip=out)
        total = out[0].clone()
    if error_if_nonfinite and not bool(torch.isfinite(total)):
        raise RuntimeError(f"The total norm of order {norm_type} for gradients from `parameters` is non-finite, so "
                           "it cannot be clipped. To disable this error and scale the gradients by the non-finite "
                           "norm anyway, set `error_if_nonfinite=False`")
    return total


def _clip_coef32(total, max_norm):
    """clip_grads_with_norm_'s coefficient lines on an fp32 0-dim tensor."""
    return torch.clamp((total + 1e-6).reciprocal() * max_norm, max=1.0)


_plans = {}  # id of a list's first parameter -> its ParamSgdPlan (which holds weak references only)


def _sgd_plan(params):
    """The cached plan of this parameter list, or None where the batched kernel does not take
    it (CPU tensors, other dtypes, non-contiguous or several devices)."""
    plan = _plans.get(id(params[0]))
    if plan is not None and plan.holds(params):
        return plan
    dev = params[0].device
    if not all(p.is_cuda and p.device == dev and p.dtype in codec.PARAM_DTYPES and p.is_contiguous()
               for p in params):
        return None
    if len(_plans) >= 64:  # plans of parameter lists long gone
        _plans.clear()
    plan = _plans[id(params[0])] = codec.ParamSgdPlan(params)
    return plan


class MasterWeights:
    """fp32 master weights of a bf16 / fp16 model: the persistent flat fp32 copy of the
    parameters the optimizer update runs on (apply_gradient(master=...), fused_step(master=...),
    dpsgd_step(master=...)), so that an update smaller than half a 16-bit ulp of a parameter is
    kept from one step to the next.  The model's parameters are the round-to-nearest-even
    narrowing of the master; the momentum buffers of a master update are fp32.

    Built by one pack of the model (widening is exact: narrow(master) == params from the start).
    Every group must hold one parameter, named once in param_names, as the reference's groups
    do; the flat layout is param_names' order.
        flat      the TensorBuffer over the master (`buffer`: its flat fp32 tensor)
        spare     a second flat buffer of the same size, allocated on first use (dpsgd_step
                  mixes into it and swaps the two)"""

    def __init__(self, param_groups, param_names):
        entries = step_entries(param_groups, param_names, "MasterWeights")
        params = [p for _, p in entries]
        if not all(p.dtype in codec.PARAM_DTYPES for p in params):
            raise RuntimeError("MasterWeights needs float32, bfloat16 or float16 parameters")
        self.param_names = list(param_names)
        self.flat = TensorBuffer([p.data for p in params], dtype=torch.float32)
        self._spare = None
        self._numel = self.flat.buffer.numel()
        self._seen = None  # entries()' last checked (param_groups, entries, device)

    @property
    def buffer(self):
        return self.flat.buffer

    @property
    def spare(self):
        if self._spare is None:
            self._spare = torch.empty_like(self.flat.buffer)
        return self._spare

    def swap(self):
        """The spare buffer becomes the master and the other way round."""
        self.flat.buffer, self._spare = self.spare, self.flat.buffer

    def entries(self, param_groups):
        """[(group, param)] in the master's order; raises where the master does not fit them
        (another layout, size or device)."""
        buf = self.flat.buffer
        if buf.dtype != torch.float32 or buf.dim() != 1 or not buf.is_contiguous() or buf.numel() != self._numel:
            raise RuntimeError(f"the master buffer must be a flat contiguous float32 tensor of {self._numel} elements")
        seen = self._seen
        # the very objects the last call checked, on the buffer's device: one pass of identity tests
        if (seen is not None and seen[0] is param_groups and seen[2] == buf.device and len(param_groups) == len(seen[1])
                and all(len(g["params"]) == 1 and g["params"][0] is p for g, p in seen[1])):
            return seen[1]
        entries = step_entries(param_groups, self.param_names, "a step with master weights")
        if ([p.size() for _, p in entries] != self.flat._tensors_sizes
                or any(p.device != buf.device for _, p in entries)):
            raise RuntimeError("the master weights do not fit this model: another layout or device")
        self._seen = (param_groups, entries, buf.device)
        return entries

    def to_model(self, param_groups):
        """The unpack: every parameter = its master slice narrowed to the parameter's dtype."""
        self.flat.unpack([p.data for _, p in self.entries(param_groups)])

    def from_model(self, param_groups):
        """The re-pack, after the model's parameters were written from outside (a checkpoint of
        the 16-bit model, a broadcast): master = the parameters widened."""
        params = [p.data for _, p in self.entries(param_groups)]
        self.flat.buffer.copy_(flatten(params, dtype=torch.float32))

    def state_dict(self):
        return {"master": self.flat.buffer}

    def load_state_dict(self, state_dict):
        src = state_dict["master"]
        if src.numel() != self.flat.buffer.numel() or src.dtype != torch.float32:
            raise RuntimeError(f"the saved master holds {src.numel()} {src.dtype} elements, this one "
                               f"{self.flat.buffer.numel()} float32")
        self.flat.buffer.copy_(src.reshape(-1))


def apply_gradient_master_loop(param_groups, state, master, write=True, grads32=None):
    """apply_gradient on master weights as one torch op per line and tensor, on fp32 views of
    the master with p.grad.float(), then p.data.copy_(view) (write): the path CPU tensors, and
    anything the batched kernel does not take, keep.  Same bits as the kernel, which in fp32 are
    apply_gradient_loop's.  grads32 (fp32 tensors in the master's order): the gradients in
    place of p.grad.float() (allreduce_sgd_step_loop's unrounded average)."""
    entries = master.entries(param_groups)
    _master_bufs_are_fp32(entries, state)
    for i, (group, p) in enumerate(entries):
        if p.grad is None:
            continue
        weight_decay, momentum = group["weight_decay"], group["momentum"]
        view = master.flat[i]
        d_p = p.grad.data.float() if grads32 is None else grads32[i]
        if weight_decay != 0:
            d_p = d_p.add(view, alpha=weight_decay)  # out of place: p.grad keeps its values
        if momentum != 0:
            param_state = state[p]
            if "momentum_buffer" not in param_state:
                buf = param_state["momentum_buffer"] = torch.zeros_like(p.data, dtype=torch.float32)
                buf.mul_(momentum).add_(d_p)
            else:
                buf = param_state["momentum_buffer"]
                buf.mul_(momentum).add_(d_p, alpha=1 - group["dampening"])
            d_p = d_p.add(buf, alpha=momentum) if group["nesterov"] else buf
        view.add_(d_p, alpha=-group["lr"])
        if write:
            p.data.copy_(view)


def _not_fp32(dtype):
    return RuntimeError(f"a step with master weights needs float32 momentum buffers, found {dtype}: convert "
                        "optimizer.state's buffers (buf.float()) when switching to master weights")


def _master_bufs_are_fp32(entries, state):
    for _, p in entries:
        buf = (state.get(p) or {}).get("momentum_buffer")
        if buf is not None and buf.dtype != torch.float32:
            raise _not_fp32(buf.dtype)


def _sgd_master(param_groups, state, master, write, clip=None, ls=None):
    """apply_gradient on the master weights: the batched launch, or the loop above for tensors
    the kernel does not take.  Raises, with nothing changed, where the master does not fit the
    model or a momentum buffer is not fp32.  clip, a (clip_norm, write_clipped, total_norm)
    tuple: global-norm clipping in front, the coefficient in fp32 and the clipped gradient not
    narrowed before the update.  ls, a (scaler, clip_norm or None, write_clipped) tuple: the
    loss-scaled step (clip is then None)."""
    entries = master.entries(param_groups)
    plan = _sgd_fill(entries, state, True, master.buffer, master=True)
    if ls is not None:
        scaler, max_norm, write_clipped = ls
        if plan is None:
            apply_gradient_scaled_loop(param_groups, state, scaler, master, max_norm, write_clipped, write)
        else:
            out = scaler.last = plan.gradnorm_scaled(scaler, max_norm, coef_dtype=torch.float32)
            if not _first_step_overflow(plan, out):
                plan.run_master(master.buffer, write, scaled=out, write_clipped=write_clipped)
        return plan
    if clip is None:
        if plan is None:
            apply_gradient_master_loop(param_groups, state, master, write)
        else:
            plan.run_master(master.buffer, write)
        return plan
    clip_norm, write_clipped, total_norm = clip
    if plan is None:
        grads = [p.grad for _, p in entries if p.grad is not None]
        grads32 = [None] * len(entries)
        if grads:
            c = _clip_coef32(_total_norm(grads, total_norm, torch.float32), clip_norm)
            for i, (_, p) in enumerate(entries):
                if p.grad is not None:
                    grads32[i] = p.grad.data.float() * c.to(p.grad.device)
        apply_gradient_master_loop(param_groups, state, master, write, grads32=grads32)
        if write_clipped:
            for (_, p), g in zip(entries, grads32):
                if g is not None:
                    p.grad.data.copy_(g)
    else:
        out = plan.gradnorm(clip_norm, coef_dtype=torch.float32, total_norm=total_norm)
        plan.run_master(master.buffer, write, gclip=out, write_clipped=write_clipped)
    return plan


def _sgd_batched(entries, state, apply_grad_to_model, flat, write, clip=None, ls=None, sr=None):
    """One batched launch (per chunk) for `entries`, a list of (group, param) in flat order.
    Returns False, with nothing changed, where a tensor cannot take it.  clip, a (clip_norm,
    write_clipped, total_norm) tuple: the norm pass in front and the clipped update.  ls, a
    (scaler, clip_norm or None, write_clipped) tuple: the loss-scaled step; a first step that
    overflowed launches the pack of the unchanged params alone.  sr, a (seed, step) pair (apply
    mode, not with ls): the stochastic-rounding kernel, which refuses fp16 tensors."""
    plan = _sgd_fill(entries, state, apply_grad_to_model, flat)
    if plan is None:
        return False
    if ls is not None:
        _run_scaled(plan, [p for _, p in entries], flat, write, ls)
    elif clip is None:
        plan.run(flat, grad_mode=not apply_grad_to_model, write=write, sr=sr)
    else:
        plan.run(flat, grad_mode=not apply_grad_to_model, write=write,
                 gclip=plan.gradnorm(clip[0], total_norm=clip[2]), write_clipped=clip[1], sr=sr)
    return True


def _run_scaled(plan, params, flat, write, ls):
    """The loss-scaled norm launch and update of a filled plan (not the master's)."""
    scaler, max_norm, write_clipped = ls
    out = scaler.last = plan.gradnorm_scaled(scaler, max_norm)
    if not _first_step_overflow(plan, out):
        plan.run(flat, write=write, scaled=out, write_clipped=write_clipped)
    elif flat is not None:
        codec.params_pack([p.data for p in params], flat)


def _clipped_loop(param_groups, state, apply_grad_to_model, clip):
    """clip_grad_norm_loop, then apply_gradient_loop.  Without write_clipped the gradients
    get their own values back in apply mode, as the batched path leaves them."""
    clip_norm, write_clipped, total_norm = clip
    params = [p for group in param_groups for p in group["params"] if p.grad is not None]
    saved = None if write_clipped or not apply_grad_to_model else [p.grad.data.clone() for p in params]
    clip_grad_norm_loop(params, clip_norm, total_norm)
    apply_gradient_loop(param_groups, state, apply_grad_to_model)
    if saved is not None:
        for p, g in zip(params, saved):
            p.grad.data.copy_(g)


def _sgd_fill(entries, state, apply_grad_to_model, flat, master=False):
    """The plan of `entries` with this step's pointers, flags and hyperparameters written (and
    missing momentum buffers created), ready to run; None, with nothing changed, where a tensor
    cannot take the batched kernels.  master: `flat` is the master copy and the momentum buffers
    are fp32 (plan.run_master follows).  plan.created: the state entries whose buffer this call
    created (a loss-scaled step that overflows takes them back, _first_step_overflow)."""
    if not entries:
        return None
    params = [p for _, p in entries]
    plan = _sgd_plan(params)
    if plan is None or (flat is not None and (flat.dtype != torch.float32 or flat.device != plan.device
                                              or flat.numel() != plan.n or not flat.is_contiguous())):
        return None
    pp, gp, bp, flags, seen = plan.param_ptrs, plan.grad_ptrs, plan.buf_ptrs, plan.flags, plan.seen
    created = []
    ok, wrong = True, None
    for i, (group, p) in enumerate(entries):
        momentum = group["momentum"]
        g = p.grad
        if g is None:
            if not apply_grad_to_model:  # the reference skips it; a flat gradient has no slot to skip
                ok = False
                break
            pp[i], gp[i], bp[i], flags[i] = p.data_ptr(), None, None, codec.SGD_F_NOGRAD
            continue
        fl = codec.SGD_F_NESTEROV if group["nesterov"] else 0
        b_ptr = None
        if momentum != 0:
            param_state = state[p]
            buf = param_state.get("momentum_buffer")
            if buf is None:  # written, not read, by its first step
                buf = torch.zeros_like(p.data, dtype=torch.float32 if master else None)
                param_state["momentum_buffer"] = buf
                created.append(param_state)
                fl |= codec.SGD_F_FIRST
            if not (plan.fits_master_buf(i, buf) if master else plan.fits(i, buf)):
                wrong = buf.dtype if master and buf.dtype != torch.float32 else None
                ok = False
                break
            b_ptr = buf.data_ptr()
        if not plan.fits(i, g):
            ok = False
            break
        pp[i], gp[i], bp[i], flags[i] = p.data_ptr(), g.data_ptr(), b_ptr, fl
        hp = (group["lr"], group["weight_decay"], momentum, group["dampening"])
        if hp != seen[i]:
            plan.lr[i], plan.weight_decay[i], plan.momentum[i], plan.dampening[i] = hp
            seen[i] = hp
    if not ok:
        for param_state in created:
            del param_state["momentum_buffer"]
        if wrong is not None:  # a 16-bit step's buffer: no silent fall-back to the loop
            raise _not_fp32(wrong)
        return None
    plan.created = created
    return plan


class LossScaler:
    """Dynamic loss scaling for fp16 (and bf16) models, torch.amp.GradScaler's rule with its
    work fused into the step: `scaler.scale(loss).backward()`, then apply_gradient / fused_step /
    dpsgd_step(..., loss_scale=scaler).  The step's norm pass tests the still scaled gradients
    for an inf or a NaN, the update multiplies by 1 / scale (times the clip coefficient) on the
    load it does anyway, an overflowed step is skipped on the device, and the scale is backed
    off or grown there too: no unscale_ pass, no found_inf.item(), no second norm pass.

    Device state: `_scale` (fp32) and `_growth_tracker` (int32), one element each.
        scale(loss)   loss * scale, a device multiply
        last          the last step's [total norm of the unscaled gradient, coefficient / scale,
                      found (1.0: the step was skipped), the scale it ran with], on the device
        get_scale(), skipped()   read the scale / last[2] on the host: the only calls that sync
    state_dict / load_state_dict use torch.amp.GradScaler's keys: its checkpoints load."""

    def __init__(self, device, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        self.device = torch.device(device)
        self._check(init_scale, growth_factor, backoff_factor, growth_interval)
        self.growth_factor, self.backoff_factor = float(growth_factor), float(backoff_factor)
        self.growth_interval = int(growth_interval)
        self._scale = torch.full((1,), float(init_scale), dtype=torch.float32, device=self.device)
        self._growth_tracker = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.last = None

    @staticmethod
    def _check(scale, growth_factor, backoff_factor, growth_interval):
        s32 = torch.tensor(float(scale), dtype=torch.float32)
        if not (bool(torch.isfinite(s32)) and float(s32) > 0.0):
            raise RuntimeError(f"LossScaler: the scale must be finite and > 0 as an fp32 value, got {scale}")
        if not (1.0 < float(growth_factor) < float("inf")):
            raise RuntimeError(f"LossScaler: growth_factor must be finite and > 1, got {growth_factor}")
        if not 0.0 < float(backoff_factor) < 1.0:
            raise RuntimeError(f"LossScaler: backoff_factor must be in (0, 1), got {backoff_factor}")
        if int(growth_interval) != growth_interval or int(growth_interval) < 1:
            raise RuntimeError(f"LossScaler: growth_interval must be an integer >= 1, got {growth_interval}")

    def scale(self, loss):
        """loss * scale on the device (no sync); the loss keeps its shape and dtype."""
        return loss * self._scale.reshape(())

    def get_scale(self):
        return float(self._scale)

    def skipped(self):
        """Whether the last step overflowed and was skipped (reads `last` on the host)."""
        return self.last is not None and bool(self.last[2] != 0)

    def state_dict(self):
        return {"scale": self.get_scale(), "growth_factor": self.growth_factor,
                "backoff_factor": self.backoff_factor, "growth_interval": self.growth_interval,
                "_growth_tracker": int(self._growth_tracker)}

    def load_state_dict(self, state_dict):
        sd = state_dict
        self._check(sd["scale"], sd["growth_factor"], sd["backoff_factor"], sd["growth_interval"])
        self.growth_factor, self.backoff_factor = float(sd["growth_factor"]), float(sd["backoff_factor"])
        self.growth_interval = int(sd["growth_interval"])
        self._scale.fill_(float(sd["scale"]))
        self._growth_tracker.fill_(int(sd["_growth_tracker"]))


def apply_gradient_scaled_loop(param_groups, state, scaler, master=None, clip_norm=None, write_clipped=False,
                               write=True):
    """The loss-scaled step (apply_gradient(loss_scale=)) as one torch op per line: the path CPU
    tensors, and anything the batched kernels do not take, keep.  The lines are the kernels'
    (include/choco_codec.h, dynamic loss scaling); the state update is torch._amp_update_scale_,
    the update apply_gradient_master_loop(grads32=) or apply_gradient_loop, and the skip is a
    host branch.  Returns [total, coefficient / scale, found, scale] (also scaler.last)."""
    if master is not None:
        params = [p for _, p in master.entries(param_groups)]
    else:
        params = [p for group in param_groups for p in group["params"]]
    grads = [p.grad for p in params if p.grad is not None]
    if not grads:
        return None
    dev = grads[0].device
    cd = torch.float32 if master is not None else codec.common_grad_dtype(g.dtype for g in grads)
    scale = scaler._scale.reshape(()).clone()
    inv = scale.double().reciprocal().float()
    ssq = torch.stack([g.detach().double().pow(2).sum().to(dev) for g in grads]).sum()
    found = (~torch.isfinite(ssq)).float()
    total = (ssq.sqrt().float() * inv).to(cd)
    c = torch.ones((), dtype=cd, device=dev) if clip_norm is None else _clip_coef32(total, clip_norm)
    gc = c.float() * inv
    out = scaler.last = torch.stack([total.float(), gc, found, scale])
    torch._amp_update_scale_(scaler._scale, scaler._growth_tracker, found.reshape(1), scaler.growth_factor,
                             scaler.backoff_factor, scaler.growth_interval)
    if bool(found):
        return out
    if master is not None:
        grads32 = [None if p.grad is None else p.grad.data.float() * gc for p in params]
        apply_gradient_master_loop(param_groups, state, master, write, grads32=grads32)
        if write_clipped:
            for p, g in zip(params, grads32):
                if g is not None:
                    p.grad.data.copy_(g)
        return out
    params = [p for p in params if p.grad is not None]
    saved = None if write_clipped else [p.grad.data.clone() for p in params]
    for p in params:
        p.grad.data.copy_(p.grad.data.float() * gc)  # one fp32 product, narrowed once
    apply_gradient_loop(param_groups, state, True)
    if saved is not None:
        for p, g in zip(params, saved):
            p.grad.data.copy_(g)
    return out


def _first_step_overflow(plan, out):
    """SGD_F_FIRST is decided on the host, from a missing momentum buffer: a step skipped on the
    device would leave a zero buffer that the next step reads as initialised (wrong whenever
    dampening != 0).  So while a step creates a buffer, `found` is read on the host -- the one
    sync of the loss-scaled path, gone from the first taken step on -- and on overflow the
    created buffers are taken back.  True: launch no update."""
    if not plan.created or not bool(out[2] != 0):
        return False
    for param_state in plan.created:
        del param_state["momentum_buffer"]
    plan.created = []
    return True


def _scale_args(what, loss_scale, clip_norm=None, write_clipped=False, total_norm=None, apply_grad_to_model=True):
    """(clip, ls) of a step: without loss_scale its _clip_args tuple and None; with it None --
    the clip is the scaled norm launch's own -- and (scaler, clip_norm or None, write_clipped)."""
    if loss_scale is None:
        return _clip_args(what, clip_norm, write_clipped, total_norm, apply_grad_to_model), None
    if not isinstance(loss_scale, LossScaler):
        raise RuntimeError(f"{what}: loss_scale must be a LossScaler")
    if not apply_grad_to_model:
        raise RuntimeError(f"{what}: loss_scale updates the model; apply_grad_to_model=False (grad mode) has no "
                           "loss-scaled variant")
    if total_norm is not None:
        raise RuntimeError(f"{what}: loss_scale with a pinned total_norm: there is no norm pass to detect an "
                           "overflow from")
    return None, (loss_scale, None if clip_norm is None else float(clip_norm), bool(write_clipped))


def _clip_args(what, clip_norm, write_clipped=False, total_norm=None, apply_grad_to_model=True):
    """The (clip_norm, write_clipped, total_norm) tuple of a clipped step, or None without one."""
    if clip_norm is None:
        if write_clipped or total_norm is not None:
            raise RuntimeError(f"{what}: write_clipped / total_norm need clip_norm")
        return None
    if write_clipped and not apply_grad_to_model:
        raise RuntimeError(f"{what}: write_clipped is for apply_grad_to_model=True; without it d_p is what the "
                           "gradients receive")
    return float(clip_norm), bool(write_clipped), total_norm


def _sr_args(what, rounding, param_groups, master=None, loss_scale=None, apply_grad_to_model=True):
    """The (seed, step) pair of a step with rounding=..., or None without.  The combinations
    stochastic rounding does not take raise before anything is changed or the stream advanced."""
    if rounding is None:
        return None
    _sr_refuse(what, param_groups, master, loss_scale, apply_grad_to_model)
    return sr_pair(rounding)


def _sr_refuse(what, param_groups, master=None, loss_scale=None, apply_grad_to_model=True):
    """Raises for the combinations a step with rounding=... does not take; touches nothing."""
    if master is not None:
        raise RuntimeError(f"{what}: rounding= (stochastic rounding) with master= -- the master weights keep small "
                           "updates already, and the parameters are their round-to-nearest narrowing")
    if loss_scale is not None:
        raise RuntimeError(f"{what}: rounding= (stochastic rounding) has no loss-scaled form: bf16 needs no loss "
                           "scale, and fp16 models use LossScaler with MasterWeights")
    if not apply_grad_to_model:
        raise RuntimeError(f"{what}: rounding= (stochastic rounding) rounds the store of a parameter; "
                           "apply_grad_to_model=False stores none")
    for group in param_groups:
        for p in group["params"]:
            if p.dtype not in (torch.bfloat16, torch.float32):
                raise RuntimeError(f"{what}: rounding= (stochastic rounding) takes bfloat16 parameters (and passes "
                                   f"float32 ones through), found {p.dtype}")


def no_rounding(what, rounding):
    """The steps stochastic rounding does not cover raise when handed it."""
    if rounding is not None:
        raise RuntimeError(f"{what}: rounding= (stochastic rounding) is not supported here -- this step's parameter "
                           "store is not the SGD update's or the unpack's; apply_gradient and the CHOCO fused_step "
                           "take it")


def apply_gradient(param_groups, state, apply_grad_to_model=True, flat_out=None, master=None, clip_norm=None,
                   write_clipped=False, total_norm=None, loss_scale=None, rounding=None):
    """optim/utils.py:13-47: weight decay, momentum with dampening, optional Nesterov, then
    p -= lr * d_p (apply_grad_to_model) or d_p left as the gradient.  Missing
    state[p]["momentum_buffer"] entries are created.  fp32 / bf16 / fp16 ROCm tensors take ONE
    batched HIP launch per chunk of tensors (codec.params_sgd); CPU tensors, and anything else,
    the per-tensor loop above.

    flat_out (a TensorBuffer or a flat fp32 tensor over every parameter, in group order): it
    receives, in the same pass, the new parameters (what recover_params' flatten would build
    next) or, with apply_grad_to_model=False, d_p (what get_data(is_get_grad=True) +
    TensorBuffer would).

    Two differences from the reference, by design: with apply_grad_to_model the grad tensors
    are never written (the reference adds the weight decay into p.grad in place); without it
    d_p is written into the existing grad tensors' storage and p.grad is not rebound to the
    momentum buffer object.

    master (a MasterWeights of this model; apply_grad_to_model only, no flat_out): the update
    runs in fp32 on the master copy, in place, and the parameters receive its values narrowed
    to their dtype -- one launch of codec.params_sgd_master per chunk.  Missing momentum
    buffers are created as fp32; an existing one of another dtype raises.

    clip_norm (conf.rnn_clip): torch.nn.utils.clip_grad_norm_(params, clip_norm) in front of the
    update (distributed_running_nlp.py:96-97), fused: one norm pass over the gradients, the
    coefficient computed on the device with torch's op sequence, and the update launch scales
    g by it on the load it does anyway.  The total norm is clip_grad_norm_'s of this module
    (fp64 accumulation over all elements); total_norm (a tensor or a float) pins it.
    p.grad is not written unless write_clipped (apply_grad_to_model only), which stores the
    clipped gradient as torch's call leaves it.  With master the coefficient is computed in
    fp32 and the clipped gradient is not narrowed before the update.

    loss_scale (a LossScaler; apply_grad_to_model only, no total_norm): the gradients are
    those of scaler.scale(loss).  The norm pass detects an inf / NaN from its fp64 sum of
    squares, the update multiplies g by (clip coefficient) / scale on the load it does anyway
    (clip_norm None: by 1 / scale), an overflowed step changes nothing -- flat_out receives the
    unchanged parameters -- and the scale is backed off or grown on the device; write_clipped
    (with or without clip_norm) stores the unscaled, clipped gradient.  Nothing is read on the
    host, except while a step creates momentum buffers (the first taken step): `found` is then
    read, and an overflowed step leaves no buffer behind.  loss_scale=None is the code path
    above, launch for launch.

    rounding (a StochasticRounding, which advances by one step, or a (seed, step) pair;
    apply_grad_to_model only, bf16 and fp32 parameters, with or without flat_out and clip_norm,
    not with master or loss_scale): the third way to train a bf16 model.  Every line up to d_p
    is as above; the parameter line stays fp32, flat_out receives it unrounded, and the ONE
    store that writes a bf16 parameter rounds stochastically, with 16 bits that are a function
    of (seed, step, flat index in group order) alone (include/choco_codec.h; sr_bits and
    sr_narrow_bf16 restate it): an update below half a bf16 ulp survives in expectation, with
    no extra memory and the plain update's traffic.  fp32 parameters get the same bits as
    without.  One launch of codec ParamSgdPlan.run(sr=) per chunk; CPU tensors take
    apply_gradient_sr_loop.  rounding=None is the code path above, launch for launch."""
    sr = _sr_args("apply_gradient", rounding, param_groups, master, loss_scale, apply_grad_to_model)
    clip, ls = _scale_args("apply_gradient", loss_scale, clip_norm, write_clipped, total_norm, apply_grad_to_model)
    if master is not None:
        if not apply_grad_to_model:
            raise RuntimeError("apply_gradient(master=...) updates the model: apply_grad_to_model=False has no "
                               "master variant")
        if flat_out is not None:
            raise RuntimeError("apply_gradient(master=...): the master buffer is the flat copy; flat_out has no use")
        _sgd_master(param_groups, state, master, write=True, clip=clip, ls=ls)
        return
    entries = [(group, p) for group in param_groups for p in group["params"]]
    flat = getattr(flat_out, "buffer", flat_out)
    if _sgd_batched(entries, state, apply_grad_to_model, flat, write=True, clip=clip, ls=ls, sr=sr):
        return
    if sr is not None:
        if flat is not None and (flat.dtype != torch.float32 or flat.dim() != 1):
            raise RuntimeError("apply_gradient(rounding=...): flat_out must be a flat float32 buffer")
        return apply_gradient_sr_loop(param_groups, state, sr[0], sr[1], clip, flat)
    if ls is not None:
        apply_gradient_scaled_loop(param_groups, state, ls[0], None, ls[1], ls[2])
    elif clip is None:
        apply_gradient_loop(param_groups, state, apply_grad_to_model)
    else:
        _clipped_loop(param_groups, state, apply_grad_to_model, clip)
    if flat is not None:
        flat.copy_(flatten([p.data if apply_grad_to_model else p.grad.data for _, p in entries], dtype=flat.dtype))


# ----------------------------------------------------------------------------- Adam / AdamW
_ADAM_REFUSED = ("amsgrad", "maximize", "capturable", "differentiable")


def _adam_hp(what, group):
    """(lr, beta1, beta2, eps, weight_decay, decoupled) of a torch.optim.Adam / AdamW group;
    raises for what the update does not take."""
    for key in _ADAM_REFUSED:
        if group.get(key, False):
            raise RuntimeError(f"{what}: {key}=True is not supported (DESIGN.md section 8, the Adam update's scope)")
    lr, (beta1, beta2) = group["lr"], group["betas"]
    if any(torch.is_tensor(x) for x in (lr, beta1, beta2)):
        raise RuntimeError(f"{what}: a tensor lr or beta is not supported -- the hyperparameters are host floats "
                           "(DESIGN.md section 8, the Adam update's scope)")
    return (float(lr), float(beta1), float(beta2), float(group["eps"]), float(group["weight_decay"]),
            bool(group.get("decoupled_weight_decay", False)))


def _adam_state(what, entries, state, master):
    """Per entry with a gradient (step tensor or None, exp_avg or None, exp_avg_sq or None) of
    what the state holds, None for the others; raises, before anything is changed, for a state
    the update does not take."""
    out = []
    for _, p in entries:
        if p.grad is None:
            out.append(None)
            continue
        st = state.get(p) or {}
        step, m, v = st.get("step"), st.get("exp_avg"), st.get("exp_avg_sq")
        if (m is None) != (v is None):
            raise RuntimeError(f"{what}: a state with one of exp_avg / exp_avg_sq and not the other")
        if step is not None and (not torch.is_tensor(step) or step.is_cuda):
            raise RuntimeError(f"{what}: state['step'] must be a CPU tensor (torch's own, without capturable): the "
                               "count is kept and incremented on the host")
        if m is None and step is not None and float(step) != 0:
            raise RuntimeError(f"{what}: a state with a step count of {float(step):g} and no moments")
        want = torch.float32 if master is not None else p.dtype
        for t in (m, v):
            if t is None or t.dtype == want:
                continue
            if master is not None:
                raise RuntimeError(f"{what}: a step with master weights needs float32 moments, found {t.dtype}: "
                                   "convert optimizer.state's exp_avg / exp_avg_sq (.float()) when switching to "
                                   "master weights")
            raise RuntimeError(f"{what}: {t.dtype} moments beside a {p.dtype} parameter need a master copy "
                               "(master=); without one the moments have the parameter's dtype (DESIGN.md section 8)")
        out.append((step, m, v))
    return out


def _adam_begin(entries, state, held, master):
    """The step's host side, once nothing can raise any more: missing step counts and moments
    are created (torch.empty: the first update writes them and does not read them) and every
    count is incremented, on the host.  Returns per entry (step after the increment, exp_avg,
    exp_avg_sq, first) or None."""
    out = []
    for (_, p), h in zip(entries, held):
        if h is None:
            out.append(None)
            continue
        st = state[p]
        step, m, v = h
        if step is None:
            step = st["step"] = torch.tensor(0.0, dtype=torch.float32)
        first = m is None
        if first:
            dt = torch.float32 if master is not None else p.dtype
            m = st["exp_avg"] = torch.empty_like(p.data, dtype=dt, memory_format=torch.preserve_format)
            v = st["exp_avg_sq"] = torch.empty_like(p.data, dtype=dt, memory_format=torch.preserve_format)
        step += 1
        out.append((float(step), m, v, first))
    return out


def _adam_lines(hp, p, g, m, v, step, first):
    """choco_params_adam's lines on one tensor, one torch op each: p (the parameter's data or
    its master view) is updated in place, g is read, m and v are updated in place."""
    lr, beta1, beta2, eps, wd, decoupled = hp
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    if first:
        m.zero_()
        v.zero_()
    if wd != 0:
        if decoupled:
            p.mul_(1 - lr * wd)
        else:
            g = g.add(p, alpha=wd)  # out of place: p.grad keeps its values
    m.lerp_(g, 1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    # the correctly rounded fp32 square root, narrowed to v's dtype: torch's CPU sqrt of a large fp32 tensor goes
    # through a vector math library that is 1 ulp off on some inputs, the float64 one rounded to fp32 is not
    den = v.double().sqrt_().float().to(v.dtype)
    den = den.div_(bc2 ** 0.5)
    den = den.add_(eps)
    q = m.div(den)
    p.add_(q, alpha=-(lr / bc1))  # q rounded, then one fused multiply-add: the kernel's line


def apply_adam_loop(param_groups, state, master=None, clip_norm=None, write_clipped=False, total_norm=None,
                    write=True):
    """apply_adam as one torch op per line and tensor: the path CPU tensors, and anything the
    batched kernel does not take, keep.  The same bits as the kernel on fp32 tensors; the
    parameter line is q = m / den rounded and then one fused multiply-add, where torch's addcdiv_
    rounds elsewhere, and the square root is taken in float64 and rounded to fp32 (the correctly
    rounded one, which torch's CPU sqrt of a large fp32 tensor is not).  With master the lines run on fp32 views of the master with
    p.grad.float(), then p.data.copy_(view) (write)."""
    what = "apply_adam_loop"
    if master is not None:
        entries = master.entries(param_groups)
    else:
        entries = [(group, p) for group in param_groups for p in group["params"]]
    hps = [_adam_hp(what, group) for group, _ in entries]
    clip = _clip_args(what, clip_norm, write_clipped, total_norm)
    held = _adam_state(what, entries, state, master)
    rows = _adam_begin(entries, state, held, master)
    with_grad = [p for _, p in entries if p.grad is not None]
    grads = {}
    if clip is not None and with_grad:
        if master is not None:  # the coefficient in fp32, the product not narrowed
            c = _clip_coef32(_total_norm([p.grad for p in with_grad], clip[2], torch.float32), clip[0])
            grads = {p: p.grad.data.float() * c.to(p.grad.device) for p in with_grad}
        else:
            saved = None if clip[1] else [p.grad.data.clone() for p in with_grad]
            clip_grad_norm_loop(with_grad, clip[0], clip[2])
    for i, ((_, p), hp, row) in enumerate(zip(entries, hps, rows)):
        if row is None:
            continue
        step, m, v, first = row
        if master is None:
            _adam_lines(hp, p.data, p.grad.data, m, v, step, first)
            continue
        view = master.flat[i]
        _adam_lines(hp, view, grads[p] if p in grads else p.grad.data.float(), m, v, step, first)
        if write:
            p.data.copy_(view)
    if clip is not None and with_grad:
        if master is not None and clip[1]:
            for p in with_grad:
                p.grad.data.copy_(grads[p])
        elif master is None and saved is not None:
            for p, g in zip(with_grad, saved):
                p.grad.data.copy_(g)


_adam_plans = {}  # id of a list's first parameter -> its ParamAdamPlan (which holds weak references only)


def _adam_plan(params):
    """The cached Adam plan of this parameter list, or None where the batched kernel does not
    take it (CPU tensors, other dtypes, non-contiguous or several devices)."""
    plan = _adam_plans.get(id(params[0]))
    if plan is not None and plan.holds(params):
        return plan
    dev = params[0].device
    if not all(p.is_cuda and p.device == dev and p.dtype in codec.PARAM_DTYPES and p.is_contiguous()
               for p in params):
        return None
    if len(_adam_plans) >= 64:  # plans of parameter lists long gone
        _adam_plans.clear()
    plan = _adam_plans[id(params[0])] = codec.ParamAdamPlan(params)
    return plan


def _adam_batched(what, entries, hps, state, flat, master, write, clip, sr=None):
    """One batched launch (per chunk) for `entries`, a list of (group, param) in flat order:
    the plan's tables are written by index, missing state is created, the counts are
    incremented and the kernel runs -- after the norm pass where clip, a (clip_norm,
    write_clipped, total_norm) tuple, is given.  flat: the flat output or None; with master the
    master's buffer.  sr, a (seed, step) pair: the stochastic-rounding update (no master); its
    clip coefficient is computed in fp32, as the master update's is.  Returns False, with
    nothing changed, where a tensor cannot take it."""
    if not entries:
        return False
    held = _adam_state(what, entries, state, master)
    plan = _adam_plan([p for _, p in entries])
    if plan is None or (flat is not None and (flat.dtype != torch.float32 or flat.device != plan.device
                                              or flat.numel() != plan.n or not flat.is_contiguous())):
        return False
    fits_moment = plan.fits_master_buf if master is not None else plan.fits
    for i, ((_, p), h) in enumerate(zip(entries, held)):
        if h is None:
            continue
        if not plan.fits(i, p.grad) or any(t is not None and not fits_moment(i, t) for t in h[1:]):
            return False
    rows = _adam_begin(entries, state, held, master)
    pp, gp, mp, vp, flags, seen = (plan.param_ptrs, plan.grad_ptrs, plan.exp_avg_ptrs, plan.exp_avg_sq_ptrs,
                                   plan.flags, plan.seen)
    for i, ((_, p), hp, row) in enumerate(zip(entries, hps, rows)):
        if row is None:
            pp[i], gp[i], mp[i], vp[i], flags[i] = p.data_ptr(), None, None, None, codec.ADAM_F_NOGRAD
            continue
        step, m, v, first = row
        pp[i], gp[i], mp[i], vp[i] = p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr()
        flags[i] = (codec.ADAM_F_DECOUPLED if hp[5] else 0) | (codec.ADAM_F_FIRST if first else 0)
        plan.step[i] = step
        if hp != seen[i]:  # an unchanged lr costs nothing
            plan.lr[i], plan.beta1[i], plan.beta2[i], plan.eps[i], plan.weight_decay[i] = hp[:5]
            seen[i] = hp
    gclip = None
    if clip is not None:
        fp32_coef = master is not None or sr is not None
        gclip = plan.gradnorm(clip[0], coef_dtype=torch.float32 if fp32_coef else None, total_norm=clip[2])
    if master is not None:
        plan.run_master(flat, write, gclip=gclip, write_clipped=clip is not None and clip[1])
    elif sr is not None:
        plan.run(flat, write, gclip=gclip, write_clipped=clip is not None and clip[1], sr=sr)
    else:
        plan.run(flat, write, gclip=gclip, write_clipped=clip is not None and clip[1])
    return True


def apply_adam(param_groups, state, flat_out=None, master=None, clip_norm=None, write_clipped=False,
               total_norm=None, rounding=None):
    """Drop-in for torch.optim.Adam.step / AdamW.step on torch's own group keys (`lr`, `betas`,
    `eps`, `weight_decay`, `decoupled_weight_decay`, default False) and state keys
    (state[p]["step"], a CPU float32 0-dim tensor incremented on the host with no sync,
    "exp_avg", "exp_avg_sq"): a torch.optim.AdamW state_dict loads into it and its state loads
    into torch.optim.AdamW.  fp32 / bf16 / fp16 ROCm tensors take ONE batched HIP launch per
    chunk of tensors (codec.params_adam: every operand read once); CPU tensors, and anything
    else, apply_adam_loop.  The arithmetic is include/choco_codec.h's: torch's op sequence with
    one rounding per line, the same bits on every path for fp32 tensors.

    Missing moments are created with torch.empty, in the parameter's dtype or, with master, in
    fp32; the first update writes them and never reads them.  `amsgrad`, `maximize`,
    `capturable`, `differentiable`, a tensor lr or beta, and moments of another dtype than the
    step's raise before anything is touched.

    flat_out (a TensorBuffer or a flat fp32 tensor over every parameter, in group order)
    receives the new parameters in the same pass.  master (a MasterWeights of this model; no
    flat_out): the update runs in fp32 on the master copy, in place, with fp32 moments, and the
    parameters receive its values narrowed to their dtype.  clip_norm / write_clipped /
    total_norm: apply_gradient's global-norm clipping, fused into the update the same way.

    rounding (a StochasticRounding, which advances by one step, or a (seed, step) pair; bf16 and
    fp32 parameters, with or without flat_out and clip_norm, not with master): Adam for a bf16
    model in the plain update's memory and traffic.  With round-to-nearest bf16 moments
    exp_avg_sq * 0.999 is exp_avg_sq again and a step of lr below half an ulp of p is lost; here
    a bf16 tensor's lines run in fp32 on the widened operands with nothing narrowed between them
    (the clip coefficient is computed in fp32 and its product not narrowed), and the stores of
    the parameter, exp_avg and exp_avg_sq round stochastically with bit fields ("lanes") 0, 1
    and 2 of (seed, step, flat index in group order) (include/choco_codec.h; sr_bits(lane=) and
    sr_narrow_bf16 restate it); flat_out receives p_new unrounded.  The moments stay bf16 under
    torch's keys, so a state of plain apply_adam or torch.optim.AdamW continues here and the
    reverse.  fp32 parameters get the same bits as without.  One launch of codec
    ParamAdamPlan.run(sr=) per chunk; CPU tensors take apply_adam_sr_loop.  rounding=None is the
    code path above, launch for launch."""
    what = "apply_adam"
    hps_of = {id(group): _adam_hp(what, group) for group in param_groups}
    clip = _clip_args(what, clip_norm, write_clipped, total_norm)
    if rounding is not None:
        _sr_refuse(what, param_groups, master)
    if master is not None:
        if flat_out is not None:
            raise RuntimeError("apply_adam(master=...): the master buffer is the flat copy; flat_out has no use")
        _adam_master(what, param_groups, state, master, True, clip)
        return
    entries = [(group, p) for group in param_groups for p in group["params"]]
    flat = getattr(flat_out, "buffer", flat_out)
    hps = [hps_of[id(group)] for group, _ in entries]
    if rounding is not None:
        _adam_sr(what, entries, hps, state, flat, True, clip, rounding)
        return
    if _adam_batched(what, entries, hps, state, flat, None, True, clip):
        return
    apply_adam_loop(param_groups, state, None, clip_norm, write_clipped, total_norm)
    if flat is not None:
        flat.copy_(flatten([p.data for _, p in entries], dtype=flat.dtype))


def _adam_master(what, param_groups, state, master, write, clip):
    """apply_adam on the master weights: the batched launch, or the loop for tensors the kernel
    does not take.  Raises, with nothing changed, where the master does not fit the model or a
    moment is not fp32."""
    entries = master.entries(param_groups)
    hps = [_adam_hp(what, group) for group, _ in entries]
    if not _adam_batched(what, entries, hps, state, master.buffer, master, write, clip):
        apply_adam_loop(param_groups, state, master, *(clip or (None, False, None)), write=write)


def _adam_packed(param_groups, param_names, state, clip):
    """fused_step(state=..., update="adam"): apply_adam and the pack of the new params in one
    launch.  Returns the flat TensorBuffer, or None after the per-tensor loop has updated the
    params (tensors the batched kernel does not take: recover_params packs them as before)."""
    what = 'fused_step(update="adam")'
    entries = step_entries(param_groups, param_names, what)
    hps = [_adam_hp(what, group) for group, _ in entries]
    dev = entries[0][1].device
    flat = torch.empty(sum(p.numel() for _, p in entries), dtype=torch.float32, device=dev)
    if dev.type == "cuda" and _adam_batched(what, entries, hps, state, flat, None, False, clip):
        return TensorBuffer.from_flat(flat, [p.size() for _, p in entries])
    apply_adam_loop(param_groups, state, None, *(clip or (None, False, None)))
    return None


def _adam_sr(what, entries, hps, state, flat, write, clip, rounding):
    """apply_adam(rounding=...) on `entries`, (group, param) in flat order: whatever can raise is
    checked first, then the stream advances once, then the batched launch runs -- or the loop,
    for tensors the kernel does not take.  Returns the (seed, step) pair it used."""
    if flat is not None and (flat.dtype != torch.float32 or flat.dim() != 1
                             or flat.numel() != sum(p.numel() for _, p in entries)):
        raise RuntimeError(f"{what}(rounding=...): flat_out must be a flat float32 buffer over every parameter")
    _adam_state(what, entries, state, None)
    sr = sr_pair(rounding)
    if not _adam_batched(what, entries, hps, state, flat, None, write, clip, sr=sr):
        _adam_sr_entries(what, entries, hps, state, sr, clip, flat, write)
    return sr


def _adam_sr_entries(what, entries, hps, state, sr, clip, flat, write):
    """apply_adam_sr_loop's body on (group, param) entries in flat order."""
    held = _adam_state(what, entries, state, None)
    for _, p in entries:
        if p.dtype not in (torch.bfloat16, torch.float32):
            raise RuntimeError(f"stochastic rounding takes bfloat16 and float32 parameters, found {p.dtype}")
    rows = _adam_begin(entries, state, held, None)
    with_grad = [p for _, p in entries if p.grad is not None]
    coef = None
    if clip is not None and with_grad:  # the coefficient in fp32, the product not narrowed: the master update's lines
        coef = _clip_coef32(_total_norm([p.grad for p in with_grad], clip[2], torch.float32), clip[0])
    off = 0
    for (_, p), hp, row in zip(entries, hps, rows):
        n = p.numel()
        if row is None:
            new = p.data.float()
        else:
            step, m, v, first = row
            g = p.grad.data.float()
            if coef is not None:
                g = g * coef.to(g.device)
                if clip[1]:
                    p.grad.data.copy_(g)
            if p.dtype == torch.float32:
                new = p.data if write else p.data.clone()
                _adam_lines(hp, new, g, m, v, step, first)
            else:
                new, m32, v32 = p.data.float(), m.float(), v.float()
                _adam_lines(hp, new, g, m32, v32, step, first)
                for t, t32, lane in ((m, m32, 1), (v, v32, 2)) + (((p.data, new, 0),) if write else ()):
                    t.copy_(sr_narrow_bf16(t32, sr_bits(sr[0], sr[1], off, n, lane=lane)).view_as(t))
        if flat is not None:
            flat[off:off + n] = new.reshape(-1)
        off += n


def apply_adam_sr_loop(param_groups, state, seed, step, clip=None, flat=None, write=True):
    """apply_adam(rounding=...) as one torch op per line and tensor: the path CPU tensors keep,
    and what the kernel is compared against.  A bf16 tensor's p, g, exp_avg and exp_avg_sq are
    widened, _adam_lines runs on the fp32 copies (nothing narrowed between the lines), and
    exp_avg, exp_avg_sq and (write) the parameter are stored through sr_narrow_bf16 with
    sr_bits(seed, step, its flat offset, its length, lane=1 / 2 / 0) -- the flat index in group
    order, as `flat` (a flat fp32 tensor over every parameter, or None) lays the parameters out;
    flat receives p_new unrounded.  An fp32 tensor takes apply_adam_loop's lines and draws no
    bits; a parameter without a gradient puts its values into flat and is not written; any other
    dtype raises.  `seed`, `step`: the rounding stream's, not the optimizer's count, which is
    state[p]["step"] as ever.  clip, a (clip_norm, write_clipped, total_norm) tuple: the
    coefficient in fp32 (_total_norm, _clip_coef32), one fp32 product per element, not narrowed
    in front of the lines; write_clipped stores it, narrowed to the gradient's dtype."""
    what = "apply_adam_sr_loop"
    entries = [(group, p) for group in param_groups for p in group["params"]]
    hps = [_adam_hp(what, group) for group, _ in entries]
    _adam_sr_entries(what, entries, hps, state, (seed, step), clip, flat, write)


def _adam_sr_packed(param_groups, param_names, state, clip, rounding):
    """fused_step(state=..., update="adam_sr"): apply_adam(rounding=) with the parameters not
    written and the pack of the unrounded p_new in one launch (the loop, for tensors the kernel
    does not take, fills the flat buffer the same way).  Returns the flat TensorBuffer and the
    (seed, step) pair the step's unpack rounds with."""
    what = 'fused_step(update="adam_sr")'
    entries = step_entries(param_groups, param_names, what)
    hps = [_adam_hp(what, group) for group, _ in entries]
    _sr_refuse(what, param_groups)
    flat = torch.empty(sum(p.numel() for _, p in entries), dtype=torch.float32, device=entries[0][1].device)
    sr = _adam_sr(what, entries, hps, state, flat, False, clip, rounding)
    return TensorBuffer.from_flat(flat, [p.size() for _, p in entries]), sr


def recover_params(param_groups, param_names, rank=None, neighbor_hat_params=None, get_hat_params=True):
    """optim/utils.py:50-64: flat copies of the params (and of x_hat_i).

    The flat buffers of an fp32 / bf16 / fp16 model are fp32, as the reference's are
    (communication.py:69-75 widens any model into the default dtype): the gossip step, the
    delta and the message are computed from the unrounded fp32 copy, and only unpack() rounds
    back to the model's precision (tensor_buffer.py:38-40)."""
    params = [_get_data(param_groups, idx, False) for idx, _ in param_names]
    params = [p for p in params if p is not None]
    floating = all(p.dtype in codec.PARAM_DTYPES for p in params)
    flatten_params = TensorBuffer(params, dtype=torch.float32 if floating else None)
    if get_hat_params:
        assert neighbor_hat_params is not None and rank is not None
        hat = torch.empty_like(flatten_params.buffer)
        hat.copy_(neighbor_hat_params[rank].buffer)
        flatten_hat_params = TensorBuffer.from_flat(hat, [p.size() for p in params])
        return params, flatten_params, flatten_hat_params
    return params, flatten_params


def fused_step(compressor, param_groups, param_names, shapes, neighbor_hat_params, neighbors_info,
               consensus_stepsize, rank, defer_receive=False, state=None, master=None, clip_norm=None,
               loss_scale=None, rounding=None, update="sgd"):
    """ParallelCHOCO_V.step after apply_gradient (parallel_choco_v.py:115-155), with the
    consensus step fused into the compressor's first pass: recover_params, then
    compress (x += gamma * (memory - x_hat_i) and d = x_new - x_hat_i in one pass), sync,
    uncompress, and the updated x unpacked into the model.  Returns the sync_buffer.
    The reference runs update_params_from_neighbor as its own pass before compress.

    defer_receive=True (QSGD, sign): this step's uncompress is applied by the NEXT step's
    compress, in the same pass as that step's consensus step (the reference's step runs
    the previous step's join, then update_params_from_neighbor, with only apply_gradient
    -- which touches x alone -- in between, parallel_choco_v.py:104-131).  x is the same
    after every step; x_hat / memory lag by one step until the next step or
    compressor.flush_receive() (call it before reading or saving them).  flatten_hat_params
    is x_hat_i itself, not a copy (the pass updates it in place).

    state (optimizer.state; default None: the caller has run apply_gradient, as above): the
    step runs apply_gradient itself, as the fused SGD + pack launch -- one pass that reads p,
    g and the momentum buffer and writes the buffer and the flat x.  The launch does not write
    the params (the unpack at the end writes them and nothing in between reads them) and
    recover_params' pack is skipped.  Every group must hold one parameter, named in
    param_names, as the reference's groups do.

    master (a MasterWeights of this model; needs state): the step's first launch is the update
    on the master copy (the params are not written), and the master's buffer is the step's
    flatten_params -- no flat buffer is allocated and nothing is packed.  Compress, gossip,
    sync and uncompress work on it as on any flat x, and the unpack at the end narrows it into
    the model.

    clip_norm (needs state; conf.rnn_clip): apply_gradient(clip_norm=...)'s global-norm
    clipping in front of the step's update.  Without state the caller has run apply_gradient
    already and there is nothing left to clip: that raises.

    loss_scale (a LossScaler; needs state): apply_gradient(loss_scale=...)'s loss-scaled
    update.  A step whose gradients overflowed leaves x as it was and goes on: the consensus
    step, the compressor and the exchange run on the unchanged x.

    rounding (a StochasticRounding or a (seed, step) pair; needs state; bf16 and fp32
    parameters; not with master or loss_scale): the step's first launch is the
    stochastic-rounding update with the parameters not written -- the flat x receives the
    unrounded fp32 p_new, so the consensus step and the compressor see no rounding at all --
    and the unpack at the end is the stochastic one.  One (seed, step) serves both, and only
    the unpack stores parameters: the whole step rounds each parameter once.

    update ("sgd", the default: everything above, launch for launch; or "adam"; needs state):
    with "adam" the groups and state are torch.optim.Adam's / AdamW's (apply_adam) and the
    step's first launch is the Adam update with the parameters not written and the flat x
    receiving p_new; with master it is the master update, and the master's buffer is x.
    clip_norm works as above.  loss_scale has no Adam form (the Adam
    update's scope) and raises, and so does rounding with "adam", whose arithmetic is torch's
    per-line bf16.

    update="adam_sr" (needs state and rounding; bf16 and fp32 parameters; not with master or
    loss_scale): apply_adam(rounding=)'s arithmetic -- fp32 lines between stochastically
    rounded bf16 stores.  The step's first launch is that update with the parameters not
    written: exp_avg and exp_avg_sq are rounded there (lanes 1 and 2) and the flat x receives
    the unrounded p_new; the consensus step, the compressor and the exchange see no rounding;
    the unpack at the end stores each parameter once (lane 0), with the same (seed, step)."""
    flatten_params = None
    if update not in ("sgd", "adam", "adam_sr"):
        raise RuntimeError(f"fused_step: update must be 'sgd', 'adam' or 'adam_sr', got {update!r}")
    if update == "adam":
        if loss_scale is not None or rounding is not None:
            raise RuntimeError("fused_step(update='adam'): loss_scale= has no Adam form -- a skipped step must not "
                               "advance the step count, which is kept on the host -- and rounding= goes with "
                               "update='adam_sr', whose fp32 lines between bf16 stores are another arithmetic than "
                               "update='adam''s per-line bf16 (DESIGN.md section 8, the Adam update's scope)")
        if state is None:
            raise RuntimeError("fused_step(update='adam') runs apply_adam itself: pass state=optimizer.state")
    if update == "adam_sr":
        if rounding is None:
            raise RuntimeError("fused_step(update='adam_sr') is the Adam update with stochastic rounding: pass "
                               "rounding= (a StochasticRounding or a (seed, step) pair); without it the update is "
                               "update='adam'")
        if state is None:
            raise RuntimeError("fused_step(update='adam_sr') runs apply_adam itself: pass state=optimizer.state")
        if loss_scale is not None:
            raise RuntimeError("fused_step(update='adam_sr'): loss_scale= has no Adam form -- a skipped step must not "
                               "advance the step count, which is kept on the host (DESIGN.md section 8, the Adam "
                               "update's scope)")
        _sr_refuse("fused_step(update='adam_sr')", param_groups, master)
    if rounding is not None and state is None:
        raise RuntimeError("fused_step(rounding=...) rounds in the step's own apply_gradient and unpack: pass "
                           "state=optimizer.state (without it the caller's apply_gradient has already rounded)")
    # update="adam_sr" advances the stream itself, once its own checks have passed (_adam_sr_packed)
    sr = None if update == "adam_sr" else _sr_args("fused_step", rounding, param_groups, master, loss_scale)
    clip, ls = _scale_args("fused_step", loss_scale, clip_norm)
    if ls is not None and state is None:
        raise RuntimeError("fused_step(loss_scale=...) unscales in the step's own apply_gradient: pass "
                           "state=optimizer.state (without it the caller's apply_gradient has already run)")
    if clip is not None and state is None:
        raise RuntimeError("fused_step(clip_norm=...) clips in front of the step's own apply_gradient: pass "
                           "state=optimizer.state (without it the caller's apply_gradient has already run)")
    if master is not None:
        if state is None:
            raise RuntimeError("fused_step(master=...) runs apply_gradient itself: pass state=optimizer.state")
        if master.param_names != list(param_names):
            raise RuntimeError("fused_step(master=...): the master weights were built for other param_names")
        if update == "adam":
            _adam_master("fused_step(update='adam')", param_groups, state, master, False, clip)
        else:
            _sgd_master(param_groups, state, master, write=False, clip=clip, ls=ls)
        flatten_params = master.flat
    elif update == "adam":
        flatten_params = _adam_packed(param_groups, param_names, state, clip)
    elif update == "adam_sr":
        flatten_params, sr = _adam_sr_packed(param_groups, param_names, state, clip, rounding)
    elif state is not None:
        flatten_params = _sgd_packed(param_groups, param_names, state, clip, ls, sr)
    if defer_receive:
        if flatten_params is None:
            params, flatten_params = recover_params(param_groups, param_names, get_hat_params=False)
        else:
            params = [_get_data(param_groups, idx, False) for idx, _ in param_names]
        flatten_hat_params = neighbor_hat_params[rank]
    else:
        if hasattr(compressor, "flush_receive"):  # a receive an earlier deferred step left
            compressor.flush_receive()
        if flatten_params is None:
            params, flatten_params, flatten_hat_params = recover_params(param_groups, param_names, rank,
                                                                        neighbor_hat_params, get_hat_params=True)
        else:
            params = [_get_data(param_groups, idx, False) for idx, _ in param_names]
            hat = torch.empty_like(flatten_params.buffer)
            hat.copy_(neighbor_hat_params[rank].buffer)
            flatten_hat_params = TensorBuffer.from_flat(hat, [p.size() for p in params])
    sync_buffer = {"original_shapes": shapes, "flatten_params": flatten_params,
                   "flatten_hat_params": flatten_hat_params,
                   "gossip": (neighbor_hat_params["memory"].buffer, consensus_stepsize)}
    if defer_receive:
        sync_buffer["defer_receive"] = True
    compressor.pipeline(sync_buffer, neighbor_hat_params, neighbors_info)
    if sr is None:
        flatten_params.unpack(params)
    else:
        flatten_params.unpack(params, rounding=sr)
    return sync_buffer


def _sgd_packed(param_groups, param_names, state, clip=None, ls=None, sr=None):
    """fused_step(state=...): apply_gradient and the pack of the new params in one launch.
    Returns the flat TensorBuffer, or None after the per-tensor loop has updated the params
    (tensors the batched kernel does not take: recover_params packs them as before).  sr, a
    (seed, step) pair: the stochastic-rounding update; its loop too leaves the params unwritten
    and returns the flat buffer of the unrounded p_new."""
    entries = step_entries(param_groups, param_names, "fused_step(state=...)")
    dev = entries[0][1].device
    flat = torch.empty(sum(p.numel() for _, p in entries), dtype=torch.float32, device=dev)
    if dev.type == "cuda" and _sgd_batched(entries, state, True, flat, write=False, clip=clip, ls=ls, sr=sr):
        return TensorBuffer.from_flat(flat, [p.size() for _, p in entries])
    if sr is not None:
        groups = [group for group, _ in entries]  # flat order is param_names' order
        apply_gradient_sr_loop(groups, state, sr[0], sr[1], clip, flat, write=False)
        return TensorBuffer.from_flat(flat, [p.size() for _, p in entries])
    if ls is not None:
        apply_gradient_scaled_loop(param_groups, state, ls[0], None, ls[1], ls[2])
    elif clip is None:
        apply_gradient_loop(param_groups, state, True)
    else:
        _clipped_loop(param_groups, state, True, clip)
    return None


def step_entries(param_groups, param_names, what, need_grads=False):
    """[(group, param)] in param_names' order for a step that runs apply_gradient itself: every
    group must hold one parameter, named once in param_names, as the reference's groups do.
    need_grads: a parameter without a gradient raises (the flat gradient buffer the reference
    builds with get_data(is_get_grad=True) has no slot for it)."""
    if len(param_names) != len(param_groups) or any(len(g["params"]) != 1 for g in param_groups) \
            or sorted(idx for idx, _ in param_names) != list(range(len(param_groups))):
        raise RuntimeError(f"{what} needs one parameter per group, each named once in param_names")
    entries = [(param_groups[idx], param_groups[idx]["params"][0]) for idx, _ in param_names]
    if need_grads:
        for idx, name in param_names:
            if param_groups[idx]["params"][0].grad is None:
                raise RuntimeError(f"{what}: parameter {name!r} has no gradient")
    return entries


def mix_sources(buffers, n, device):
    """Whether codec.params_mix takes `buffers` (flat tensors) as its sources for a layout of n
    elements on `device`."""
    return (device.type == "cuda" and 1 <= len(buffers) <= 64
            and all(b.is_cuda and b.device == device and b.dtype == torch.float32 and b.numel() == n
                    and b.is_contiguous() for b in buffers))


def grad_step_plan(entries, state, neighbor_hat_params):
    """The first line of DCD_PSGD.step / ECD_PSGD.step, apply_gradient(apply_grad_to_model=False),
    as the batched launch where the mix kernel can follow it: returns the plan whose tables the
    mix reuses, or None, with nothing changed, where the kernels do not take the tensors (CPU
    tensors, other dtypes, replicas that are not flat fp32 buffers of the model's size)."""
    params = [p for _, p in entries]
    hats = [h.buffer for h in neighbor_hat_params.values()]
    if not mix_sources(hats, sum(p.numel() for p in params), params[0].device):
        return None
    plan = _sgd_fill(entries, state, False, None)
    if plan is not None:
        plan.run(None, grad_mode=True, write=True)
    return plan


def weighted_sum(buffers, weights):
    """sum([b * w for ...]): the reference's own expression, one torch op per term."""
    return sum([b * w for b, w in zip(buffers, weights)])


def dpsgd_step_loop(param_groups, param_names, state, aggregator, clip=None, ls=None):
    """dpsgd_step as the reference's op sequence (sgd.py:94-121), one torch op per line: the path
    CPU tensors, and anything the batched kernels do not take, keep."""
    if ls is not None:
        apply_gradient_scaled_loop(param_groups, state, ls[0], None, ls[1], ls[2])
    elif clip is None:
        apply_gradient_loop(param_groups, state, True)
    else:
        _clipped_loop(param_groups, state, True, clip)
    params, flatten_params = recover_params(param_groups, param_names, get_hat_params=False)
    flatten_params.buffer = aggregator._agg(flatten_params.buffer, op="weighted")
    flatten_params.unpack(params)
    return get_n_bits(flatten_params.buffer)


def dpsgd_step(param_groups, param_names, state, aggregator, neighbors_info, master=None, clip_norm=None,
               loss_scale=None, rounding=None):
    """The decentralized branch of SGD.step (sgd.py:94-121), plain D-PSGD: apply_gradient fused
    with the pack of the new params (one launch; the params themselves are not written yet),
    the exchange of the flat fp32 buffer (_agg(op="get_raw_sync_data")), and ONE mix launch
    that writes sum(x_r * w_r) straight into the params (communication.py:271-277 and the
    unpack of sgd.py:118).  Returns n_bits.  Tensors the kernels do not take run
    dpsgd_step_loop.

    master (a MasterWeights of this model): the update runs on the master copy in place, the
    master buffer is what the neighbours exchange, and the mix writes the params and, in fp32,
    the master's spare buffer (sources and destination never alias); the two buffers are then
    swapped.

    clip_norm (conf.rnn_clip): apply_gradient(clip_norm=...)'s global-norm clipping in front of
    the update.

    loss_scale (a LossScaler): apply_gradient(loss_scale=...)'s loss-scaled update.  A worker
    whose gradients overflowed keeps its x and still exchanges and mixes it: each worker skips
    on its own.

    rounding: not supported (the mix kernel stores the parameters); anything but None raises."""
    no_rounding("dpsgd_step", rounding)
    clip, ls = _scale_args("dpsgd_step", loss_scale, clip_norm)
    entries = step_entries(param_groups, param_names, "dpsgd_step")
    params = [p for _, p in entries]
    dev = params[0].device
    if master is not None:
        if master.param_names != list(param_names):
            raise RuntimeError("dpsgd_step(master=...): the master weights were built for other param_names")
        plan = _sgd_master(param_groups, state, master, write=False, clip=clip, ls=ls)
        flat = master.buffer
        if plan is None:  # the loop ran: the reference's op sequence on the master
            master.flat.buffer = aggregator._agg(flat, op="weighted")
            master.flat.unpack(params)
            return get_n_bits(flat)
        local_data = aggregator._agg(flat, op="get_raw_sync_data")
        plan.mix(list(local_data.values()), [neighbors_info[r] for r in local_data], mode=codec.MIX_WRITE_PARAMS,
                 flat_out=master.spare)
        master.swap()
        return get_n_bits(flat)
    flat = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=dev)
    plan = _sgd_fill(entries, state, True, flat)
    if plan is None:
        return dpsgd_step_loop(param_groups, param_names, state, aggregator, clip, ls)
    if ls is not None:
        _run_scaled(plan, params, flat, False, ls)
    elif clip is None:
        plan.run(flat, grad_mode=False, write=False)
    else:
        plan.run(flat, grad_mode=False, write=False, gclip=plan.gradnorm(clip[0]))
    local_data = aggregator._agg(flat, op="get_raw_sync_data")
    srcs = list(local_data.values())
    weights = [neighbors_info[r] for r in local_data]
    # the running sum of more than one launch's sources needs a flat buffer of its own
    run = torch.empty_like(flat) if len(srcs) > 8 else None
    plan.mix(srcs, weights, mode=codec.MIX_WRITE_PARAMS, flat_out=run)
    return get_n_bits(flat)


def _allreduce_entries(param_groups, param_names, master):
    entries = step_entries(param_groups, param_names, "allreduce_sgd_step", need_grads=True)
    if master is not None:
        if master.param_names != list(param_names):
            raise RuntimeError("allreduce_sgd_step(master=...): the master weights were built for other param_names")
        entries = master.entries(param_groups)
    return entries


def _apply_averaged_loop(entries, state, grads):
    """apply_gradient_loop's lines (apply mode) with grads[i] as the gradient of entry i, each
    line one torch op in fp32 on the widened operands and one narrowing to the tensor's dtype:
    the kernels' documented model.  For fp32 tensors the widening and the narrowing are no-ops
    and these are apply_gradient_loop's very ops.  For 16-bit tensors torch's own ops are not
    that model everywhere: an fp16 op on the device rounds the exact result once, a 16-bit op on
    the CPU rounds the product before the sum."""
    for (group, p), g in zip(entries, grads):
        p.data.copy_(_update_lines(group, p, g, state).to(p.dtype))


def _update_lines(group, p, g, state):
    """_apply_averaged_loop's lines for one tensor with gradient g, up to the parameter line,
    which is returned in fp32, not yet narrowed: p_new = p + (-lr) * d_p.  The momentum buffer
    is written (and created)."""
    weight_decay, momentum = group["weight_decay"], group["momentum"]
    dt = p.dtype
    d_p = g.data
    if weight_decay != 0:
        d_p = d_p.float().add(p.data.float(), alpha=weight_decay).to(dt)
    if momentum != 0:
        param_state = state[p]
        first = "momentum_buffer" not in param_state
        if first:
            param_state["momentum_buffer"] = torch.zeros_like(p.data)
        buf = param_state["momentum_buffer"]
        t = buf.float().mul(momentum).to(dt)                                   # buf.mul_(momentum)
        t = t.float().add(d_p.float(), alpha=1 if first else 1 - group["dampening"]).to(dt)  # .add_(d_p, alpha=)
        buf.copy_(t)
        d_p = d_p.float().add(buf.float(), alpha=momentum).to(dt) if group["nesterov"] else buf
    return p.data.float().add(d_p.float(), alpha=-group["lr"])


def apply_gradient_sr_loop(param_groups, state, seed, step, clip=None, flat=None, write=True):
    """apply_gradient(rounding=...) as one torch op per line and tensor: the path CPU tensors
    keep, and what the kernel is compared against.  Every line up to d_p is _update_lines'
    (fp32 on the widened operands, narrowed to the tensor's dtype after each line); the
    parameter line stays fp32, `flat` (a flat fp32 tensor over every parameter in group order,
    or None) receives it unrounded, and a bf16 parameter (write) is stored through
    sr_narrow_bf16 with sr_bits(seed, step, its flat offset, its length) -- the flat index in
    group order, as flat lays the parameters out.  An fp32 parameter receives p_new itself;
    a parameter without a gradient puts its values into flat and is not written; any other
    dtype raises.  clip, a (clip_norm, write_clipped, total_norm) tuple: global-norm clipping in
    front, the kernel's lines -- the total (_total_norm) and the coefficient (_clip_coef32) in the
    gradients' common dtype, then one fp32 product per element narrowed once to the gradient's
    dtype; without write_clipped the gradients get their own values back."""
    params = [p for group in param_groups for p in group["params"]]
    for p in params:
        if p.dtype not in (torch.bfloat16, torch.float32):
            raise RuntimeError(f"stochastic rounding takes bfloat16 and float32 parameters, found {p.dtype}")
    saved = None
    with_grad = [p for p in params if p.grad is not None]
    if clip is not None and with_grad:
        clip_norm, write_clipped, total_norm = clip
        saved = None if write_clipped else [(p, p.grad.data.clone()) for p in with_grad]
        grads = [p.grad for p in with_grad]
        cd = codec.common_grad_dtype(g.dtype for g in grads)
        gc = _clip_coef32(_total_norm(grads, total_norm, cd), clip_norm).float()
        for g in grads:
            g.data.copy_(g.data.float() * gc.to(g.device))
    off = 0
    for group in param_groups:
        for p in group["params"]:
            n = p.numel()
            if p.grad is None:
                new = p.data.float()
            else:
                new = _update_lines(group, p, p.grad, state)
                if write and p.dtype == torch.bfloat16:
                    p.data.copy_(sr_narrow_bf16(new, sr_bits(seed, step, off, n)))
                elif write:
                    p.data.copy_(new)
            if flat is not None:
                flat[off:off + n] = new.reshape(-1)
            off += n
    if saved is not None:
        for p, g in saved:
            p.grad.data.copy_(g)


def _allreduce_scaled_loop(entries, param_groups, state, aggregator, distributed, write_grads, master, clip, ls):
    """allreduce_sgd_step_loop with clip_norm and / or loss_scale: the kernels' lines
    (include/choco_codec.h, clip and loss scale in the pack), one torch op each."""
    grads = [p.grad.data for _, p in entries]
    dev = grads[0].device
    cd = torch.float32 if master is not None else codec.common_grad_dtype(g.dtype for g in grads)
    found = None
    if ls is not None:
        scaler, clip_norm = ls[0], ls[1]
        scale = scaler._scale.reshape(()).clone()
        inv = scale.double().reciprocal().float()
        ssq = torch.stack([g.detach().double().pow(2).sum().to(dev) for g in grads]).sum()
        found = (~torch.isfinite(ssq)).float()
        total = (ssq.sqrt().float() * inv).to(cd)
        c = torch.ones((), dtype=cd, device=dev) if clip_norm is None else _clip_coef32(total, clip_norm)
        gc = c.float() * inv
        out = scaler.last = torch.stack([total.float(), gc, found, scale])
    else:
        gc = _clip_coef32(_total_norm(grads, clip[2], cd), clip[0]).float()
    # the pack: one fp32 product per element, narrowed once to the gradient's dtype unless master
    packed = [g.float() * gc if master is not None else (g.float() * gc).to(g.dtype).float() for g in grads]
    n = sum(g.numel() for g in grads)
    flat = torch.cat([x.reshape(-1) for x in packed] + ([] if found is None else [found.reshape(1)]))
    flat = aggregator._agg(flat, op="sum", distributed=distributed)
    n_bits = get_n_bits(flat)
    if ls is not None:
        found = (flat[n:] != 0).float()
        out[2] = found[0]
        torch._amp_update_scale_(scaler._scale, scaler._growth_tracker, found, scaler.growth_factor,
                                 scaler.backoff_factor, scaler.growth_interval)
        if bool(found):
            return n_bits
    divisor = float(aggregator.world_size) if distributed else 1.0
    avg = flat[:n].div(torch.full((), divisor, dtype=flat.dtype, device=flat.device))
    flatten_grads = TensorBuffer.from_flat(avg, [g.shape for g in grads])
    if master is not None:
        apply_gradient_master_loop(param_groups, state, master, write=True,
                                   grads32=[flatten_grads[i] for i in range(len(entries))])
        if write_grads:
            flatten_grads.unpack(grads)
    else:
        avg = grads if write_grads else [torch.empty_like(g) for g in grads]  # p.grad keeps its values
        flatten_grads.unpack(avg)
        _apply_averaged_loop(entries, state, avg)
    return n_bits


def allreduce_sgd_step_loop(param_groups, param_names, state, aggregator, distributed=True, write_grads=True,
                            master=None, clip_norm=None, total_norm=None, loss_scale=None):
    """allreduce_sgd_step as the reference's op sequence (sgd.py:69-92), one torch op per line:
    TensorBuffer(grads) in fp32, the all-reduce, the division by the world size, the unpack into
    the grads, apply_gradient_loop's lines (_apply_averaged_loop: for fp32 tensors the same ops;
    16-bit tensors are widened for each line).  The path CPU tensors, and anything the batched
    kernels do not take, keep; same bits as the kernels.  _agg(op="avg") is written out as _agg(op="sum")
    and one division by a 0-dim tensor: on CPU tensors the same bits, and on the device a true
    division too (torch multiplies a device tensor by the reciprocal of a Python scalar).

    master: the division's fp32 result is the gradient of apply_gradient_master_loop's lines,
    unrounded, and is then narrowed into p.grad (write_grads).

    clip_norm / total_norm / loss_scale: allreduce_sgd_step's, with the kernels' lines -- the
    coefficient (_clip_coef32) and, with loss_scale, apply_gradient_scaled_loop's inv / found /
    total / gc lines on the local gradients, one fp32 product per element in the pack, the
    local flag as element n of the flat buffer, torch._amp_update_scale_ on the summed flag
    and a host branch for the skip."""
    clip, ls = _scale_args("allreduce_sgd_step", loss_scale, clip_norm, False, total_norm)
    entries = _allreduce_entries(param_groups, param_names, master)
    if master is not None:
        _master_bufs_are_fp32(entries, state)
    if clip is not None or ls is not None:
        return _allreduce_scaled_loop(entries, param_groups, state, aggregator, distributed, write_grads, master,
                                      clip, ls)
    grads = [p.grad.data for _, p in entries]
    floating = all(g.dtype in codec.PARAM_DTYPES for g in grads)
    flatten_grads = TensorBuffer(grads, dtype=torch.float32 if floating else None)
    flatten_grads.buffer = aggregator._agg(flatten_grads.buffer, op="sum", distributed=distributed)
    divisor = float(aggregator.world_size) if distributed else 1.0
    flatten_grads.buffer.div_(torch.full((), divisor, dtype=flatten_grads.buffer.dtype,
                                         device=flatten_grads.buffer.device))
    if master is not None:
        apply_gradient_master_loop(param_groups, state, master, write=True,
                                   grads32=[flatten_grads[i] for i in range(len(entries))])
        if write_grads:
            flatten_grads.unpack(grads)
    else:
        avg = grads if write_grads else [torch.empty_like(g) for g in grads]  # p.grad keeps its values
        flatten_grads.unpack(avg)
        _apply_averaged_loop(entries, state, avg)
    return get_n_bits(flatten_grads.buffer)


def allreduce_sgd_step(param_groups, param_names, state, aggregator, distributed=True, write_grads=True, master=None,
                       clip_norm=None, total_norm=None, loss_scale=None, rounding=None):
    """The centralized branch of SGD.step (sgd.py:68-92), plain all-reduce data-parallel SGD, end
    to end: ONE pack launch per chunk of the gradients into a flat fp32 buffer (16-bit
    gradients are widened, which is exact), aggregator._agg(flat, op="sum",
    distributed=distributed), and ONE update launch per chunk of 72 tensors
    (codec.params_sgd_flatgrad) that divides the sum by aggregator.world_size (1.0 when not
    distributed; a true division), narrows the average into each gradient's dtype and runs
    apply_gradient's lines on it.  Returns n_bits of the flat fp32 gradient buffer.  Only
    _agg(op="sum") and .world_size of the aggregator are used: this package's
    CentralizedAggregation and the reference's both serve.  Every group must hold one parameter
    with a gradient, named once in param_names, as the reference's groups do.  Tensors the
    kernels do not take run allreduce_sgd_step_loop.

    write_grads (default): p.grad's storage receives the averaged gradient, as the reference's
    unflatten leaves it; False skips that store.  Two differences from the reference, by design:
    its later in-place weight decay on p.grad is not reproduced (as with apply_gradient), and
    p.grad is written in its own dtype's storage, never rebound.

    master (a MasterWeights of this model): the update runs in fp32 on the master copy in place,
    on the unrounded average, with fp32 momentum buffers (created as such; one of another dtype
    raises), and the parameters receive the new master values narrowed
    (codec.params_sgd_flatgrad(master=...)); p.grad receives the average narrowed.

    clip_norm (conf.rnn_clip): torch.nn.utils.clip_grad_norm_(params, clip_norm) on the LOCAL
    gradients in front of the step (distributed_running_nlp.py:96, each rank by its own norm),
    fused: one norm pass (codec ParamSgdPlan.gradnorm; total_norm pins the total), and the
    pack multiplies by the coefficient on the load it does anyway, narrowing the product once
    to the gradient's dtype (with master: the fp32 coefficient and the fp32 product, not
    narrowed).  No pass rewrites the gradients.

    loss_scale (a LossScaler; no total_norm): the gradients are those of
    scaler.scale(loss).  The norm pass finds this rank's inf / NaN without touching the
    scaler's state, the pack multiplies by (clip coefficient) / scale and puts the local flag
    into ONE extra fp32 slot behind the flat gradient, the same all-reduce sums it, one small
    launch (codec ParamSgdPlan.loss_scale_update) turns the sum into the ranks' common flag
    (scaler.last[2]) and backs the scale off or grows it, and the update skips the step on the
    device where the flag is set: every rank skips together and every scale stays in step.
    On a taken step p.grad (write_grads) receives the averaged, unscaled, clipped gradient; on
    a skipped one nothing is written but the scaler's state and `last`.  n_bits counts the
    n + 1 elements sent.  Nothing is read on the host, except while a step creates momentum
    buffers (the first taken step): the summed flag is then read after the all-reduce, and
    an overflowed step leaves no buffer behind and launches no update.

    With all three None this is the code path above, launch for launch.

    rounding: not supported (the flat-gradient kernels store the parameters); anything but
    None raises."""
    no_rounding("allreduce_sgd_step", rounding)
    clip, ls = _scale_args("allreduce_sgd_step", loss_scale, clip_norm, False, total_norm)
    entries = _allreduce_entries(param_groups, param_names, master)
    plan = _sgd_fill(entries, state, True, None if master is None else master.buffer, master=master is not None)
    if plan is None:
        return allreduce_sgd_step_loop(param_groups, param_names, state, aggregator, distributed, write_grads, master,
                                       clip_norm, total_norm, loss_scale)
    divisor = float(aggregator.world_size) if distributed else 1.0
    mbuf = None if master is None else master.buffer
    cd = None if master is None else torch.float32
    if ls is not None:
        scaler = ls[0]
        out = scaler.last = plan.gradnorm_scaled(scaler, ls[1], coef_dtype=cd, update_state=False)
        flat = torch.empty(plan.n + 1, dtype=torch.float32, device=plan.device)
        plan.pack_grads(flat, coef=out, found=out, round=master is None)
        flat = aggregator._agg(flat, op="sum", distributed=distributed)
        plan.loss_scale_update(scaler, flat)
        # SGD_F_FIRST is a host decision (_first_step_overflow): the one sync, gone from the first taken step on
        if plan.created and bool(flat[plan.n] != 0):
            for param_state in plan.created:
                del param_state["momentum_buffer"]
            plan.created = []
        else:
            plan.run_flatgrad(flat, divisor, write=True, write_grads=write_grads, master=mbuf, found_slot=True)
        return get_n_bits(flat)
    flat = torch.empty(plan.n, dtype=torch.float32, device=plan.device)
    if clip is None:
        plan.pack_grads(flat)
    else:
        plan.pack_grads(flat, coef=plan.gradnorm(clip[0], coef_dtype=cd, total_norm=clip[2]), round=master is None)
    flat = aggregator._agg(flat, op="sum", distributed=distributed)
    plan.run_flatgrad(flat, divisor, write=True, write_grads=write_grads, master=mbuf)
    return get_n_bits(flat)


def update_params_from_neighbor(neighbor_hat_params, flatten_params, consensus_stepsize, self_rank):
    """optim/utils.py:67-72:  x += gamma * (memory - x_hat_i), one fused HIP pass."""
    codec.gossip_step(flatten_params.buffer, neighbor_hat_params["memory"].buffer,
                      neighbor_hat_params[self_rank].buffer, consensus_stepsize)
