"""The Python side of the low-rank (PowerSGD) entry points (csrc/lowrank.hip; ranks 8, 16 and 32 run
csrc/lowrank_mfma.hip's matrix-instruction kernels behind the same calls).  codec.py re-exports
`LowRankPlan` and `LOWRANK_RANKS`; powersgd.py is the step built on them."""
import ctypes

import torch

from . import _lib
from . import codec as _c

LOWRANK_RANKS = (1, 2, 4, 8, 16, 32)
LOWRANK_ORTH_METHODS = ("mgs", "cholqr")
_HDR = 16  # header words of the table; then one {compressed, P / tail offset, Q offset, flat offset} row per tensor


def matrix_rows(shape):
    """The `rows` entry of a tensor's shape for the table: its first dimension, or 0 for a
    tensor of fewer than two dimensions (never compressed)."""
    return int(shape[0]) if len(shape) >= 2 else 0


class LowRankPlan:
    """The tile table of one parameter layout at one rank (include/choco_codec.h,
    choco_lowrank_plan), built once on the host and uploaded once, and the four launches that
    read it.  shapes: the tensors' shapes in layout order.

    .compressed    per tensor, whether it travels as rank-r factors
    .msg1_len      [P_0 | P_1 | .. | uncompressed elements];  .p_off: per tensor, where its P
                   (or, uncompressed, its elements) starts in message 1
    .msg2_len      [Q_0 | Q_1 | ..];  .q_off: per tensor, where its Q starts (-1: uncompressed)
    """

    def __init__(self, shapes, rank, device):
        L = _c.lib()
        self.shapes = [tuple(int(d) for d in s) for s in shapes]
        self.rank, self.device = int(rank), torch.device(device)
        self.nseg = len(self.shapes)
        self.lens = [int(torch.Size(s).numel()) for s in self.shapes]
        self.rows = [matrix_rows(s) if m else 0 for s, m in zip(self.shapes, self.lens)]
        self.n = sum(self.lens)
        p_rows, self._rows_keep = _lib.i64_array(self.rows)
        p_lens, self._lens_keep = _lib.i64_array(self.lens)
        plen = L.choco_lowrank_plan_len(p_rows, p_lens, self.nseg, self.rank)
        if plen < 0:
            raise RuntimeError(f"choco_lowrank_plan_len failed: {_lib.last_error()}")
        self._plan_host = (ctypes.c_int64 * int(plen))()
        self.plan_host = ctypes.cast(self._plan_host, ctypes.POINTER(ctypes.c_int64))
        if L.choco_lowrank_plan(p_rows, p_lens, self.nseg, self.rank, self.plan_host) != plen:
            raise RuntimeError(f"choco_lowrank_plan failed: {_lib.last_error()}")
        table = list(self._plan_host)
        self.msg1_len, self.msg2_len, self.tail_off = table[5], table[6], table[7]
        rows = [table[_HDR + 4 * t:_HDR + 4 * t + 4] for t in range(self.nseg)]
        self.compressed = [bool(r[0]) for r in rows]
        self.p_off = [r[1] for r in rows]
        self.q_off = [r[2] for r in rows]
        self.ws_bytes = int(L.choco_lowrank_workspace_size(self.plan_host))
        self.orth_ws_bytes = int(L.choco_lowrank_orth_workspace_size(self.plan_host))  # 0 under rank 8
        self.plan_dev = torch.tensor(table, dtype=torch.int64, device=self.device)

    def _flat(self, t, numel, name):
        _c._require(t, torch.float32, name)
        if t.device != self.plan_dev.device or t.numel() != numel:
            raise RuntimeError(f"{name} must hold {numel} elements on {self.plan_dev.device}")
        return _c._ptr(t)

    def _tail(self):
        dev = self.plan_dev.device
        return self.plan_host, _c._ptr(self.plan_dev), self.n, self.rank, _c._stream(dev)

    def project(self, g, e, q, msg1):
        """M = g + e over e, P = M Q into msg1, the uncompressed gradients into its tail."""
        _lib.check(_c.lib().choco_lowrank_project(self._flat(g, self.n, "g"), self._flat(e, self.n, "e"),
                                                  self._flat(q, self.msg2_len, "q"),
                                                  self._flat(msg1, self.msg1_len, "msg1"), self.msg1_len,
                                                  self.msg2_len, *self._tail()), "choco_lowrank_project")

    def orthogonalize(self, msg1, method="mgs"):
        """Orthogonalise every (summed) P of msg1 in place.  "mgs": modified Gram-Schmidt, one workgroup a
        matrix.  "cholqr" (ranks 8, 16 and 32): Cholesky-QR on the fp64 matrix instruction, three launches
        over every 256-row block (csrc/lowrank_cholqr.hip), with a workspace of its own."""
        if method == "mgs":
            _lib.check(_c.lib().choco_lowrank_orthogonalize(self._flat(msg1, self.msg1_len, "msg1"), self.msg1_len,
                                                            *self._tail()), "choco_lowrank_orthogonalize")
        elif method == "cholqr":
            ws = _c.workspace(self.plan_dev.device, "lowrank_orth", self.orth_ws_bytes)
            _lib.check(_c.lib().choco_lowrank_orthogonalize_cholqr(self._flat(msg1, self.msg1_len, "msg1"), self.msg1_len,
                                                                   _c._ptr(ws), ws.numel(), *self._tail()),
                       "choco_lowrank_orthogonalize_cholqr")
        else:
            raise RuntimeError(f"LowRankPlan.orthogonalize: method must be one of {LOWRANK_ORTH_METHODS}, got {method!r}")

    def backproject(self, e, msg1, msg2):
        """Q = M^T P^ into msg2 (M: what project left in e)."""
        ws = _c.workspace(self.plan_dev.device, "lowrank", self.ws_bytes)
        _lib.check(_c.lib().choco_lowrank_backproject(self._flat(e, self.n, "e"), self._flat(msg1, self.msg1_len, "msg1"),
                                                      self.msg1_len, self._flat(msg2, self.msg2_len, "msg2"),
                                                      self.msg2_len, _c._ptr(ws), ws.numel(), *self._tail()),
                   "choco_lowrank_backproject")

    def decode(self, e, msg1, msg2, flat_out, divisor):
        """flat_out = P^ Q^T (uncompressed: msg1's tail), e = M - flat_out / divisor."""
        _lib.check(_c.lib().choco_lowrank_decode(self._flat(e, self.n, "e"), self._flat(msg1, self.msg1_len, "msg1"),
                                                 self.msg1_len, self._flat(msg2, self.msg2_len, "msg2"), self.msg2_len,
                                                 self._flat(flat_out, self.n, "flat_out"), float(divisor),
                                                 *self._tail()), "choco_lowrank_decode")
