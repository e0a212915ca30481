"""numpy-only float64 restatement of the reference's EASE (algorithms/linear_algs.py:149-161) -- the expected values
of tests/test_ease.py, which holds it to the g12 goldens on the CPU.

    G = X^T X;  G[diag] += int(lam);  P = inv(G);  B = P / (-diag(P));  B[diag] = 0;  pred = X @ B

`X @ B` is scipy's csr @ dense: row u is ((0 + B[i1, :]) + B[i2, :]) + ... over the user's items in ascending order;
score_rows() adds in that order.  The inverse is a parameter: numpy.linalg.inv (the reference's) or a Cholesky solve,
whose distance from each other is the yardstick of what a third elimination order may differ by."""
import numpy as np


def gram(X, lam):
    """X dense 0/1 [n_users, n_items] -> X^T X + int(lam) I (exact in float64)."""
    G = X.T @ X
    G[np.diag_indices(G.shape[0])] += int(lam)
    return G


def inv_numpy(G):
    return np.linalg.inv(G)


def inv_cholesky(G):
    from scipy.linalg import cho_factor, cho_solve
    return cho_solve(cho_factor(G), np.eye(G.shape[0]))


def inv_refined(G, steps=3):
    """np.longdouble Newton-Schulz refinement P <- P (2 I - G P) of numpy's inverse (small matrices only)."""
    Gl = G.astype(np.longdouble)
    P = np.linalg.inv(G).astype(np.longdouble)
    two_i = 2 * np.eye(G.shape[0], dtype=np.longdouble)
    for _ in range(steps):
        P = P @ (two_i - Gl @ P)
    return P


def weights(P):
    B = P / (-np.diag(P))
    B[np.diag_indices(P.shape[0])] = 0
    return B


def fit(X, lam, inverse=inv_numpy):
    return weights(inverse(gram(X, lam)))


def score_rows(users, indptr, indices, B, absolute=False):
    """Rows of X @ B for `users`, added in the CSR's stored (ascending) order from 0.0; absolute=True gives |X| |B|,
    the scale the rounding error of such a row is measured against."""
    out = np.zeros((len(users), B.shape[1]))
    W = np.abs(B) if absolute else B
    for q, u in enumerate(users):
        acc = out[q]
        for i in indices[indptr[u]:indptr[u + 1]]:
            acc = acc + W[i]
        out[q] = acc
    return out


def separated(masked_scores, scale_rows, k=100, window=1e-10):
    """Per row: no two adjacent of the k + 1 largest masked scores are closer than window * the row's largest scale
    entry, so an error far below the window cannot change the top-k ids or their order."""
    top = -np.sort(-masked_scores, axis=1)[:, :k + 1]
    gaps = top[:, :-1] - top[:, 1:]
    return gaps.min(axis=1) >= window * scale_rows.max(axis=1)
