"""Cholesky-QR orthogonalisation in plain numpy (include/choco_codec.h, choco_lowrank_orthogonalize_cholqr): the Gram
matrix in blocks of 256 rows, the pivot rule, T = L^-T D, the product.  `dtype` restates the same lines in fp32;
`order=-1` visits the Gram blocks in descending order (the summation-order noise)."""
import numpy as np

EPS, TAU, BLOCK = 1e-8, 2.0 ** -30, 256


def orthogonalize(P, dtype=np.float64, order=1):
    P = P.astype(dtype)
    r = P.shape[1]
    G, L, X = (np.zeros((r, r), dtype) for _ in range(3))
    for b in range(0, P.shape[0], BLOCK)[::order]:
        G += P[b:b + BLOCK].T @ P[b:b + BLOCK]
    for k in range(r):
        s = G[k:, k].copy()
        for j in range(k):
            s -= L[k:, j] * L[k, j]
        if s[0] > dtype(TAU) * G[k, k]:  # else dropped: L_kk = 0 and nothing below it
            L[k, k] = np.sqrt(s[0])
            L[k + 1:, k] = s[1:] / L[k, k]
    for c in range(r):  # X = L^-1 by forward substitution, column c; a dropped row is zero
        for i in range(c, r):
            s = dtype(i == c)
            for j in range(c, i):
                s -= L[i, j] * X[j, c]
            X[i, c] = s / L[i, i] if L[i, i] > 0 else dtype(0)
    d = L.diagonal()
    return P @ (X.T * np.where(d > 0, d / (d + dtype(EPS)), dtype(0)))
