"""Drop-in for dl_code/pcode/utils/tensor_buffer.py (flat buffer + per-tensor views).

Difference from the reference: the flat buffer keeps the dtype of the packed
tensors (the reference's `flatten` always allocates the default float dtype,
communication.py:69-72, which silently turns int64 indices into fp32) unless
`dtype=` asks for another one: `dtype=torch.float32` is the reference's own rule
for a model's parameters, whatever their precision.

Packing fp32 / bf16 / fp16 ROCm tensors into an fp32 buffer, and unpacking such a
buffer, is one batched HIP launch per direction (codec.params_pack /
params_unpack) in place of one copy per tensor, with the same bits.
"""
import torch

from . import codec
from .rounding import sr_bits, sr_narrow_bf16, sr_pair


def _batched(tensors, buffer):
    """Whether the batched kernels can move `tensors` to / from `buffer`."""
    if buffer.dtype != torch.float32 or not buffer.is_cuda or not buffer.is_contiguous() or len(tensors) == 0:
        return False
    return all(t.device == buffer.device and t.dtype in codec.PARAM_DTYPES and t.is_contiguous() for t in tensors)


def flatten(tensors, shapes=None, use_cuda=True, dtype=None):
    pointers = [0]
    if shapes is not None:
        for shape in shapes:
            pointers.append(pointers[-1] + shape[1])
    else:
        for tensor in tensors:
            pointers.append(pointers[-1] + tensor.nelement())
    dev = tensors[0].device if (tensors[0].is_cuda and use_cuda) else "cpu"
    vec = torch.empty(pointers[-1], dtype=tensors[0].dtype if dtype is None else dtype, device=dev)
    if (len(pointers) == len(tensors) + 1 and _batched(tensors, vec)
            and all(e - s == t.nelement() for t, s, e in zip(tensors, pointers[:-1], pointers[1:]))):
        codec.params_pack(tensors, vec)
        return vec
    for tensor, start, end in zip(tensors, pointers[:-1], pointers[1:]):
        vec[start:end] = tensor.data.view(-1)
    return vec


class TensorBuffer:
    def __init__(self, tensors, use_cuda=True, dtype=None):
        indices = [0]
        for tensor in tensors:
            indices.append(indices[-1] + tensor.nelement())
        self._start_idx = indices[:-1]
        self._end_idx = indices[1:]
        self._tensors_len = len(tensors)
        self._tensors_sizes = [x.size() for x in tensors]
        self.buffer = flatten(tensors, use_cuda=use_cuda, dtype=dtype)  # copies

    @classmethod
    def from_flat(cls, buffer, sizes):
        """Wrap an existing flat buffer (no copy) with per-tensor sizes."""
        self = cls.__new__(cls)
        indices = [0]
        for s in sizes:
            n = 1
            for d in s:
                n *= d
            indices.append(indices[-1] + n)
        self._start_idx = indices[:-1]
        self._end_idx = indices[1:]
        self._tensors_len = len(sizes)
        self._tensors_sizes = [torch.Size(s) for s in sizes]
        self.buffer = buffer
        return self

    def __getitem__(self, index):
        return self.buffer[self._start_idx[index]:self._end_idx[index]].view(self._tensors_sizes[index])

    def __len__(self):
        return self._tensors_len

    def is_cuda(self):
        return self.buffer.is_cuda

    def nelement(self):
        return self.buffer.nelement()

    def unpack(self, tensors, rounding=None):
        """rounding (a rounding.StochasticRounding, which advances by one step, or a
        (seed, step) pair): bf16 tensors receive the stochastic rounding of their fp32 slice
        with the bits of (seed, step, flat index), fp32 tensors the copy; anything else raises.
        None: round to nearest, as before."""
        tensors = list(tensors)
        if rounding is not None:  # refused before the stream advances
            if self.buffer.dtype != torch.float32:
                raise RuntimeError("unpack(rounding=...) needs a float32 flat buffer")
            for i, t in enumerate(tensors):
                if t.dtype not in (torch.bfloat16, torch.float32):
                    raise RuntimeError(f"unpack(rounding=...): tensor {i} is {t.dtype}; stochastic rounding takes "
                                       "bfloat16 (and passes float32 through)")
        sr = sr_pair(rounding)
        if (len(tensors) == self._tensors_len and self._end_idx[-1:] == [self.buffer.nelement()]
                and _batched(tensors, self.buffer)
                and all(t.size() == s for t, s in zip(tensors, self._tensors_sizes))):
            codec.params_unpack(self.buffer, tensors, sr=sr)
            return
        for i, (tensor, entry) in enumerate(zip(tensors, self)):
            if sr is not None and tensor.dtype == torch.bfloat16:
                entry = sr_narrow_bf16(entry, sr_bits(sr[0], sr[1], self._start_idx[i], entry.numel()))
            tensor.data[:] = entry
