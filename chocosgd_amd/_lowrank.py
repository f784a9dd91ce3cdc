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


GOSSIP_MAX_WIDTH = 8  # n_edges * rank the batched PowerGossip kernels serve


class LowRankGossipPlan:
    """PowerGossip's five launches for a worker with `n_edges` neighbours (include/choco_codec.h, "low-rank
    gossip"; csrc/lowrank_gossip.hip): every pass over the flat parameters x serves all edges.  It owns the
    LowRankPlan table of the layout at `rank` (.table: lengths and offsets).  Per-edge buffers are flat,
    edge-major: q, dq, msg2 hold n_edges * msg2_len elements, msg1 n_edges * msg1_len, phat n_edges * p_total.
    lo_mask: bit e set where this worker is the low end of edge e.  n_edges * rank > 8 raises."""

    def __init__(self, shapes, rank, n_edges, device):
        self.table = LowRankPlan(shapes, rank, device)
        self.rank, self.n_edges = self.table.rank, int(n_edges)
        if self.rank > 4 or not 1 <= self.n_edges or self.n_edges * self.rank > GOSSIP_MAX_WIDTH:
            raise RuntimeError(f"LowRankGossipPlan: n_edges * rank must be in [1, {GOSSIP_MAX_WIDTH}] at rank 1, 2 or 4, got "
                               f"{n_edges} edges at rank {rank} (DESIGN.md section 8)")
        t = self.table
        self.n, self.msg1_len, self.msg2_len, self.p_total = t.n, t.msg1_len, t.msg2_len, t.tail_off
        self.ws_bytes = int(_c.lib().choco_lowrank_gossip_workspace_size(t.plan_host, self.n_edges))

    def _e(self, t, per_edge, name):
        return self.table._flat(t, self.n_edges * per_edge, name)

    def _tail(self):
        t = self.table
        return t.plan_host, _c._ptr(t.plan_dev), t.n, t.rank, self.n_edges, _c._stream(t.plan_dev.device)

    def project(self, x, q, msg1):
        """msg1[e] = [X Q_e | the uncompressed tensors of x] for every edge; x is read once."""
        _lib.check(_c.lib().choco_lowrank_gossip_project(self.table._flat(x, self.n, "x"), self._e(q, self.msg2_len, "q"),
                                                         self._e(msg1, self.msg1_len, "msg1"), self.msg1_len,
                                                         self.msg2_len, *self._tail()), "choco_lowrank_gossip_project")

    def orthogonalize(self, msg1_own, msg1_recv, phat, lo_mask):
        """phat[e] = Gram-Schmidt of P_e(lo end) - P_e(hi end)."""
        _lib.check(_c.lib().choco_lowrank_gossip_orthogonalize(self._e(msg1_own, self.msg1_len, "msg1_own"),
                                                               self._e(msg1_recv, self.msg1_len, "msg1_recv"),
                                                               self.msg1_len, self._e(phat, self.p_total, "phat"),
                                                               int(lo_mask), *self._tail()),
                   "choco_lowrank_gossip_orthogonalize")

    def backproject(self, x, phat, msg2):
        """msg2[e] = X^T phat[e] for every edge; x is read once."""
        ws = _c.workspace(self.table.plan_dev.device, "lowrank_gossip", self.ws_bytes)
        _lib.check(_c.lib().choco_lowrank_gossip_backproject(self.table._flat(x, self.n, "x"),
                                                             self._e(phat, self.p_total, "phat"), self.msg1_len,
                                                             self._e(msg2, self.msg2_len, "msg2"), self.msg2_len,
                                                             _c._ptr(ws), ws.numel(), *self._tail()),
                   "choco_lowrank_gossip_backproject")

    def diff(self, msg2_own, msg2_recv, q, dq, lo_mask):
        """dq[e] = Q'_e(lo end) - Q'_e(hi end); q[e] takes it, matrix by matrix, unless it is all zeros."""
        _lib.check(_c.lib().choco_lowrank_gossip_diff(self._e(msg2_own, self.msg2_len, "msg2_own"),
                                                      self._e(msg2_recv, self.msg2_len, "msg2_recv"), self.msg1_len,
                                                      self.msg2_len, self._e(q, self.msg2_len, "q"),
                                                      self._e(dq, self.msg2_len, "dq"), int(lo_mask), *self._tail()),
                   "choco_lowrank_gossip_diff")

    def apply(self, x, phat, dq, msg1_recv, weights, lo_mask):
        """x += sum_e c_e phat[e] dq[e]^T (c_e = -w_e at the low end, +w_e at the high end); uncompressed
        tensors: x += sum_e w_e (msg1_recv[e]'s tail - x).  One read-modify-write pass over x."""
        if len(weights) != self.n_edges:
            raise RuntimeError(f"LowRankGossipPlan.apply: {self.n_edges} weights expected, got {len(weights)}")
        w = (ctypes.c_double * self.n_edges)(*[float(v) for v in weights])
        _lib.check(_c.lib().choco_lowrank_gossip_apply(self.table._flat(x, self.n, "x"), self._e(phat, self.p_total, "phat"),
                                                       self._e(dq, self.msg2_len, "dq"),
                                                       self._e(msg1_recv, self.msg1_len, "msg1_recv"), self.msg1_len,
                                                       self.msg2_len, w, int(lo_mask), *self._tail()),
                   "choco_lowrank_gossip_apply")


GOSSIP_WIDE_MAX_WIDTH = 32  # n_edges * rank the matrix-instruction PowerGossip kernels serve


class LowRankGossipWidePlan(LowRankGossipPlan):
    """LowRankGossipPlan's five launches where it refuses: any rank of LOWRANK_RANKS with n_edges * rank <= 32 and
    (n_edges * rank > 8 or rank >= 8), on the fp32 matrix instruction (include/choco_codec.h, "low-rank gossip,
    wide"; csrc/lowrank_gossip_mfma.hip).  The same buffers, layouts, signatures and lo_mask; anything else raises."""

    def __init__(self, shapes, rank, n_edges, device):
        self.table = t = LowRankPlan(shapes, rank, device)
        self.rank, self.n_edges = t.rank, int(n_edges)
        width = self.n_edges * self.rank
        if self.n_edges < 1 or width > GOSSIP_WIDE_MAX_WIDTH or (width <= GOSSIP_MAX_WIDTH and self.rank < 8):
            raise RuntimeError(f"LowRankGossipWidePlan: n_edges * rank must be in ({GOSSIP_MAX_WIDTH}, "
                               f"{GOSSIP_WIDE_MAX_WIDTH}], or rank at least 8, got {n_edges} edges at rank {rank} "
                               "(DESIGN.md section 8)")
        self.n, self.msg1_len, self.msg2_len, self.p_total = t.n, t.msg1_len, t.msg2_len, t.tail_off
        self.ws_bytes = int(_c.lib().choco_lowrank_gossip_wide_workspace_size(t.plan_host, self.n_edges))

    def _call(self, name, *args):
        _lib.check(getattr(_c.lib(), "choco_lowrank_gossip_wide_" + name)(*args, *self._tail()),
                   "choco_lowrank_gossip_wide_" + name)

    def project(self, x, q, msg1):
        self._call("project", self.table._flat(x, self.n, "x"), self._e(q, self.msg2_len, "q"),
                   self._e(msg1, self.msg1_len, "msg1"), self.msg1_len, self.msg2_len)

    def orthogonalize(self, msg1_own, msg1_recv, phat, lo_mask):
        self._call("orthogonalize", self._e(msg1_own, self.msg1_len, "msg1_own"), self._e(msg1_recv, self.msg1_len, "msg1_recv"),
                   self.msg1_len, self._e(phat, self.p_total, "phat"), int(lo_mask))

    def backproject(self, x, phat, msg2):
        ws = _c.workspace(self.table.plan_dev.device, "lowrank_gossip", self.ws_bytes)
        self._call("backproject", self.table._flat(x, self.n, "x"), self._e(phat, self.p_total, "phat"), self.msg1_len,
                   self._e(msg2, self.msg2_len, "msg2"), self.msg2_len, _c._ptr(ws), ws.numel())

    def diff(self, msg2_own, msg2_recv, q, dq, lo_mask):
        self._call("diff", self._e(msg2_own, self.msg2_len, "msg2_own"), self._e(msg2_recv, self.msg2_len, "msg2_recv"),
                   self.msg1_len, self.msg2_len, self._e(q, self.msg2_len, "q"), self._e(dq, self.msg2_len, "dq"), int(lo_mask))

    def apply(self, x, phat, dq, msg1_recv, weights, lo_mask):
        if len(weights) != self.n_edges:
            raise RuntimeError(f"LowRankGossipWidePlan.apply: {self.n_edges} weights expected, got {len(weights)}")
        w = (ctypes.c_double * self.n_edges)(*[float(v) for v in weights])
        self._call("apply", self.table._flat(x, self.n, "x"), self._e(phat, self.p_total, "phat"),
                   self._e(dq, self.msg2_len, "dq"), self._e(msg1_recv, self.msg1_len, "msg1_recv"), self.msg1_len,
                   self.msg2_len, w, int(lo_mask))
