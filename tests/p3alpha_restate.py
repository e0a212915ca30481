"""numpy-only float64 restatement of P3alpha -- the expected values of tests/test_p3alpha.py, which holds it to the g13
goldens (written by the reference) on the CPU.  Written from the formulas, not from the reference's text:

    w = 1 / degree (0 where the degree is 0)
    S[i, j] = sum_u X[u, i] w_u X[u, j]          gram
    W[i, j] = w_i S[i, j]                        weights
    pred[u, j] = (w_u sum_{i in items(u)} W[i, j]) ^ alpha      score_rows, added in stored order from 0.0

Every term is positive, so any two summation orders agree to a relative (T + const) 2^-53, T = (X X^T X)[u, j] the
number of three-step paths -- rtol() states the bound the tests use."""
import numpy as np


def inv_degrees(deg):
    w = np.zeros(len(deg), np.float64)
    nz = np.asarray(deg) > 0
    w[nz] = 1.0 / np.asarray(deg, np.float64)[nz]
    return w


def gram(X, w_u):
    """X dense 0/1 [n_users, n_items], w_u [n_users] -> S = X^T diag(w_u) X, each entry added in ascending user order
    from 0.0 (sequential, so that an entry with one common user is that user's weight bitwise)."""
    n = X.shape[1]
    S = np.zeros((n, n))
    for u in np.flatnonzero(w_u > 0):
        items = np.flatnonzero(X[u])
        S[np.ix_(items, items)] += w_u[u]
    return S


def counts(X):
    """Integer co-occurrence counts X^T X (every partial sum is an integer below 2^53: the float64 product is exact)."""
    return np.rint(X.T @ X).astype(np.int64)


def weights(S, w_i):
    return w_i[:, None] * S


def score_rows(users, indptr, indices, W, w_u, alpha):
    """Rows of pred for `users`: the rows of W picked by the user's items added in stored order from 0.0, times w_u,
    to the power alpha (alpha == 1: no power is taken)."""
    out = np.zeros((len(users), W.shape[1]))
    for q, u in enumerate(users):
        acc = out[q]
        for i in indices[indptr[u]:indptr[u + 1]]:
            acc = acc + W[i]
        acc = w_u[u] * acc
        out[q] = acc if alpha == 1.0 else np.power(acc, alpha)
    return out


def paths(X):
    """T = X X^T X as exact integers: the number of three-step paths user -> item -> user -> item (every partial sum
    is an integer below 2^53, so the float64 products are exact)."""
    T = X @ (X.T @ X)
    assert T.max() < 2.0 ** 53
    return np.rint(T).astype(np.int64)


def rtol(alpha, t_max):
    """Relative bound between two correct evaluations of an entry with at most t_max paths: each side's sum is off by
    at most about (T + 6) 2^-53 relative, the power multiplies that by alpha, and the two pows add 16 + 1 ulp."""
    return 2.0 ** -52 * (max(1.0, alpha) * (t_max + 8) + 17)


def separated(masked, k=100, window=1e-9):
    """Per row: the k + 1 largest masked scores are all > 0 and each adjacent pair differs by >= window x the larger,
    so an error far below the window cannot change the top-k ids or their order."""
    top = -np.sort(-masked, axis=1)[:, :k + 1]
    ok = np.all(top > 0, axis=1)
    with np.errstate(invalid='ignore'):
        gaps = top[:, :-1] - top[:, 1:]
        ok &= np.all(gaps >= window * top[:, :-1], axis=1)
    return ok
