"""Stochastic rounding for bf16 models: the host restatement of the bit stream and of the
rounding the kernels use (include/choco_codec.h, "stochastic rounding for bf16 models"), and the
host-side counter a training loop carries.  Written from the header's definition, in numpy's
uint64 arithmetic (which wraps modulo 2^64), not from the kernels."""
import numpy as np
import torch

_M64 = (1 << 64) - 1
_GAMMA = np.uint64(0x9E3779B97F4A7C15)


def _mix(z):
    """SplitMix64's output function on a uint64 array."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def sr_key(seed, step):
    """key = mix(seed + (step + 1) * 0xD1B54A32D192ED03), a Python int."""
    z = (int(seed) + (int(step) + 1) * 0xD1B54A32D192ED03) & _M64
    return int(_mix(np.array([z], dtype=np.uint64))[0])


def sr_lane_key(seed, step, lane=0):
    """The key of bit field `lane` of (seed, step): lane 0's is sr_key(seed, step) itself, lane
    L > 0's is mix(key_0 + L * 0xD1B54A32D192ED03), a Python int."""
    key, lane = sr_key(seed, step), int(lane)
    if lane < 0:
        raise RuntimeError(f"sr_lane_key: lane must be >= 0, got {lane}")
    if lane == 0:
        return key
    return int(_mix(np.array([(key + lane * 0xD1B54A32D192ED03) & _M64], dtype=np.uint64))[0])


def sr_bits(seed, step, start, n, lane=0):
    """The 16 random bits of flat elements start .. start + n - 1 in step `step` of stream
    `seed`, a uint16 numpy array: w = mix(key + ((i >> 2) + 1) * gamma), bits
    [16 (i & 3), 16 (i & 3) + 16) of it.  Element i's bits do not depend on `start`.  lane: the
    bit field of a step that rounds several values per element (the Adam update: 0 the
    parameter, 1 exp_avg, 2 exp_avg_sq); key is sr_lane_key(seed, step, lane), lane 0 the stream
    every other caller draws."""
    i = np.arange(int(start), int(start) + int(n), dtype=np.uint64)
    w = _mix(np.uint64(sr_lane_key(seed, step, lane)) + ((i >> np.uint64(2)) + np.uint64(1)) * _GAMMA)
    return ((w >> (np.uint64(16) * (i & np.uint64(3)))) & np.uint64(0xFFFF)).astype(np.uint16)


def sr_narrow_bf16(x_fp32, bits):
    """x (an fp32 tensor, any device) narrowed to bf16 with the random bits `bits` (uint16, one
    per element, sr_bits'): inf is kept and a NaN becomes the quiet NaN 0x7fc0, as the
    round-to-nearest narrowing of the kernels has it; every other value is (bits(x) + r16) >> 16 -- the truncation or its successor in
    magnitude, the successor with probability low16 / 65536.  Returns a bf16 tensor of x's
    shape on x's device."""
    if x_fp32.dtype != torch.float32:
        raise RuntimeError(f"sr_narrow_bf16 needs a float32 tensor, got {x_fp32.dtype}")
    x = x_fp32.detach().cpu().contiguous()
    u = x.reshape(-1).numpy().view(np.uint32)
    r = np.asarray(bits).reshape(-1).astype(np.uint32)
    if r.size != u.size:
        raise RuntimeError(f"sr_narrow_bf16: {u.size} elements, {r.size} bit fields")
    mag = u & np.uint32(0x7FFFFFFF)
    out = ((u + r) >> np.uint32(16)).astype(np.uint16)
    out = np.where(mag == np.uint32(0x7F800000), (u >> np.uint32(16)).astype(np.uint16), out)  # inf kept
    out = np.where(mag > np.uint32(0x7F800000), np.uint16(0x7FC0), out)                         # the quiet NaN
    out = torch.from_numpy(out.astype(np.uint16).view(np.int16).copy()).view(torch.bfloat16)
    return out.reshape(x_fp32.shape).to(x_fp32.device)


def sr_pair(rounding):
    """(seed, step) of a step: a StochasticRounding advances (next()), a pair is taken as it is."""
    if rounding is None:
        return None
    if hasattr(rounding, "next"):
        return rounding.next()
    seed, step = rounding
    return int(seed) & _M64, int(step) & _M64


class StochasticRounding:
    """The stochastic-rounding stream of a training run: a seed and a host-side step counter.
    next() returns (seed, step) and advances; hand the object as rounding= to apply_gradient /
    fused_step / TensorBuffer.unpack, which call next() once per step.  No device state, no
    sync.  state_dict / load_state_dict (two ints): a resumed run continues its stream."""

    def __init__(self, seed, step=0):
        self.seed, self.step = int(seed) & _M64, int(step) & _M64

    def next(self):
        pair = (self.seed, self.step)
        self.step = (self.step + 1) & _M64
        return pair

    def state_dict(self):
        return {"seed": self.seed, "step": self.step}

    def load_state_dict(self, state_dict):
        self.seed, self.step = int(state_dict["seed"]) & _M64, int(state_dict["step"]) & _M64
