"""Rank-r PowerSGD in plain numpy (include/choco_codec.h, "low-rank compression"): the layout
rule, modified Gram-Schmidt, and one whole step.  `dtype` restates the same lines in fp32."""
import numpy as np

EPS = 1e-8
# the kernel tests' layout: uncompressed tensors interleaved; odd cols; 2049 = one over the LDS
# column block and over the rows orthogonalise stages; 257 = one over the back-project slab
SHAPES = [(7,), (9, 11), (), (64, 147), (0,), (7, 257), (5, 5), (300, 9), (5, 2049), (257, 6), (2049, 5), (16, 3, 3, 3)]


def numel(shape):
    return int(np.prod(shape, dtype=np.int64))


def is_compressed(shape, r):
    if len(shape) < 2 or numel(shape) == 0:
        return False
    rows, cols = shape[0], numel(shape) // shape[0]
    return rows * cols > r * (rows + cols)


class Layout:
    """Per tensor: .comp, .off (flat), .rc (rows, cols), .p_off (in message 1; the tail offset of
    an uncompressed tensor), .q_off (in message 2, -1); .n, .msg1_len, .msg2_len."""

    def __init__(self, shapes, r):
        self.shapes, self.r = [tuple(s) for s in shapes], r
        self.comp = [is_compressed(s, r) for s in self.shapes]
        self.rc = [(s[0], numel(s) // s[0]) if c else (0, 0) for s, c in zip(self.shapes, self.comp)]
        self.lens = [numel(s) for s in self.shapes]
        self.off = [sum(self.lens[:t]) for t in range(len(self.lens))]
        self.n = sum(self.lens)
        tail = sum(rows * r for rows, _ in self.rc)
        self.p_off, self.q_off, p, q = [], [], 0, 0
        for (rows, cols), c, m in zip(self.rc, self.comp, self.lens):
            self.p_off.append(p if c else tail)
            self.q_off.append(q if c else -1)
            p, q, tail = p + rows * r, q + cols * r, tail + (0 if c else m)
        self.msg1_len, self.msg2_len = tail, q

    def matrices(self):
        """(flat slice, P slice of message 1, Q slice of message 2, rows, cols) per compressed tensor."""
        for o, p, q, (rows, cols), c in zip(self.off, self.p_off, self.q_off, self.rc, self.comp):
            if c:
                yield slice(o, o + rows * cols), slice(p, p + rows * self.r), slice(q, q + cols * self.r), rows, cols

    def tails(self):
        """(flat slice, message 1 slice) per uncompressed tensor."""
        return [(slice(o, o + m), slice(p, p + m)) for o, p, m, c in zip(self.off, self.p_off, self.lens, self.comp) if not c]


def orthogonalize(P, dtype=np.float64):
    P = P.astype(dtype).copy()
    for k in range(P.shape[1]):
        P[:, k] /= dtype(np.sqrt((P[:, k] * P[:, k]).sum(dtype=dtype))) + dtype(EPS)
        for j in range(k + 1, P.shape[1]):
            P[:, j] -= (P[:, k] * P[:, j]).sum(dtype=dtype) * P[:, k]
    return P


def step(L, g, e, q, W=1.0, dtype=np.float64):
    """One step at world 1 (the all-reduces are identities): returns (sum, e', q')."""
    g, e, q = g.astype(dtype), e.astype(dtype).copy(), q.astype(dtype).copy()
    out = g.copy()
    for f, _, qs, rows, cols in L.matrices():
        M = (g[f] + e[f]).reshape(rows, cols)
        Ph = orthogonalize(M @ q[qs].reshape(cols, L.r), dtype)
        Q = M.T @ Ph
        q[qs], out[f] = Q.reshape(-1), (Ph @ Q.T).reshape(-1)
        e[f] = M.reshape(-1) - out[f] / dtype(W)
    return out, e, q
