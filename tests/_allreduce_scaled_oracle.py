"""The model of the all-reduce SGD step with a global-norm clip and / or dynamic loss scaling
(include/choco_codec.h, "clip and loss scale in the pack"), composed from _lscale_oracle (inv,
found, total, out, unscale, update), _gclip_oracle (coef, clip) and _allreduce_oracle (step,
master_step, fdiv).  Per rank, CD = the gradients' common dtype (fp32 with master weights):

    clip only:  [total, c]            = _gclip_oracle on the local gradients
    scaled:     [total, gc, found, s] = _lscale_oracle.out on the local, still scaled gradients
    the pack:   flat[i] = to_grid(coef * g, DT)     round (the fp32 / 16-bit step)
                flat[i] = coef * g                  fp32, not narrowed (the master step)
                flat[n] = found ? 1 : 0             scaled only: the flag slot
    the ranks' flats are added, then
    scaled:     found = gsum[n] != 0 (a NaN counts); _lscale_oracle.update on (scale, tracker);
                found: nothing else changes
    the update: _allreduce_oracle.step / master_step on gsum[0..n)
"""
import numpy as np

import _allreduce_oracle as AO
import _gclip_oracle as GO
import _lscale_oracle as LO
from _sgd_oracle import F32, mul32, to_grid


def pack(g, coef, dtype, round=True):
    """The pack's line: one fp32 product, narrowed once to the gradient's dtype (round) or not."""
    return GO.clip(g, coef, dtype if round else "fp32")


def coef_dtype(dtypes, master):
    return "fp32" if master else GO.common_dtype(dtypes)


def local_out(grads, dtypes, master, clip_norm=None, scale=None, total=None):
    """What this rank's norm launch leaves: [total, c] (scale None) or [total, gc, found, scale].
    total: a total on CD's grid in place of the model's own (the device's, or a pinned one)."""
    cd = coef_dtype(dtypes, master)
    if scale is None:
        t = GO.total(grads, cd) if total is None else to_grid(np.array([total], F32), cd)[0]
        return np.array([t, GO.coef(t, clip_norm, cd)], dtype=F32)
    t = LO.total(grads, scale, cd) if total is None else F32(total)
    return LO.out(t, clip_norm, scale, LO.found(grads), cd)


def rank_flat(grads, dtypes, out, master):
    """This rank's flat buffer as it enters the all-reduce: n elements, or n + 1 with the flag."""
    parts = [pack(g, out[1], dt, round=not master) for g, dt in zip(grads, dtypes)]
    if len(out) == 4:
        parts.append(np.array([out[2]], dtype=F32))
    return np.concatenate(parts) if parts else np.zeros(0, F32)


def add(flats):
    """The all-reduce SUM in the given order, one fp32 addition each."""
    s = np.asarray(flats[0], F32).copy()
    with np.errstate(all="ignore"):
        for q in flats[1:]:
            s = (s + np.asarray(q, F32)).astype(F32)
    return s


class Model:
    """One rank's model, momentum buffers, master copy and loss-scale state."""

    def __init__(self, p0, dtypes, hps, master, scale=None, growth=2.0, backoff=0.5, interval=2000):
        self.dtypes, self.hps, self.master = list(dtypes), list(hps), master
        self.lens = [int(np.size(p)) for p in p0]
        self.n = sum(self.lens)
        self.cur = [to_grid(p, dt) for p, dt in zip(p0, dtypes)]  # the master copy, or the parameters
        self.p16 = [c.copy() for c in self.cur]
        self.g16 = [None] * len(self.lens)
        self.bufs = [None] * len(self.lens)
        self.scale = None if scale is None else F32(scale)
        self.tracker = 0
        self.amp = (growth, backoff, interval)

    def local(self, grads, clip_norm=None, total=None):
        return local_out(grads, self.dtypes, self.master, clip_norm, self.scale, total)

    def flat(self, grads, out):
        return rank_flat(grads, self.dtypes, out, self.master)

    def apply(self, gsum, world):
        """The step after the all-reduce.  Returns whether it was taken."""
        if self.scale is not None:
            assert gsum.size == self.n + 1
            found = not (gsum[self.n] == 0)
            self.scale, self.tracker = LO.update(self.scale, self.tracker, found, *self.amp)
            if found:
                return False
        o = 0
        for i, m in enumerate(self.lens):
            s, dt, hp = gsum[o:o + m], self.dtypes[i], self.hps[i]
            o += m
            first = self.bufs[i] is None
            if self.master:
                self.cur[i], self.bufs[i], self.p16[i], self.g16[i] = AO.master_step(self.cur[i], s, self.bufs[i], world,
                                                                                    *hp, first=first, dtype=dt)
            else:
                self.cur[i], self.bufs[i], self.g16[i] = AO.step(self.cur[i], s, self.bufs[i], world, *hp, first=first,
                                                                 dtype=dt)
                self.p16[i] = self.cur[i]
        return True

    def cat(self, what):
        v = [x for x in getattr(self, what) if x is not None]
        return np.concatenate(v) if v else np.zeros(0, F32)
