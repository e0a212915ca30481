"""numpy-only float64 restatement of the SLIM solver law -- the expected values of
tests/test_slim.py.

The reference (algorithms/linear_algs.py:14-128) fits, per item j, sklearn's ElasticNet(positive=True,
fit_intercept=False, tol=1e-4) on X with column j zeroed, drawing coordinates at random.  Its iterates cannot be
reproduced; the problem it solves can.  With n = n_users, G = X^T X, l1 = n alpha rho and l2 = n alpha (1 - rho) that
problem is (sklearn's objective times n)

    P_j(w) = 1/2 ||x_j - X~ w||^2 + l1 sum(w) + 1/2 l2 ||w||^2,   w >= 0,   X~ = X with column j zeroed,

and solve() walks it by cyclic coordinate descent on G alone: full sweeps over i = 0 .. n_items - 1 in ascending order
(i = j and items nobody holds are skipped), every operation rounded on its own, and sklearn's duality gap as the stop
test.  The law has no reductions except inside the gap, so the iterates are order-free: the device's are these bits.
No candidate shortcut is taken here; that the shortcut changes nothing is what the device tests show.
"""
import numpy as np

TOL = 1e-4


def penalties(n_users, alpha, l1_ratio):
    """(l1, l2) of the law from the reference's hyper-parameters."""
    return n_users * alpha * l1_ratio, n_users * alpha * (1 - l1_ratio)


def gram(X):
    """X dense 0/1 [n_users, n_items] -> X^T X (exact in float64)."""
    X = np.asarray(X, np.float64)
    return X.T @ X


def gap(G, j, w, q, l1, l2):
    """sklearn's duality gap of column j at w (q_i = sum_{k != j} G_ik w_k), over the visited coordinates."""
    g, d, yy = G[j], np.diag(G), G[j, j]
    visited = d > 0
    visited[j] = False
    s = g - q - l2 * w
    D = s[visited].max() if visited.any() else -np.inf
    R2 = yy - 2 * (w @ g) + w @ q
    Ry = yy - w @ g
    if D > l1:
        c = l1 / D
        out = 0.5 * R2 * (1 + c * c)
    else:
        c = 1.0
        out = R2
    return out + (l1 * w.sum() - c * Ry + 0.5 * l2 * (1 + c * c) * (w @ w))


def gap_of(G, j, w, l1, l2):
    """The gap recomputed from a returned w alone."""
    col = G.copy()
    col[:, j] = 0
    return gap(G, j, w, col @ w, l1, l2)


def solve(G, j, l1, l2, tol, max_iter, trace=None):
    """(w, n_iter, gap) of column j.  trace, if a list, receives (sweep, i) for every coordinate that changed."""
    n = G.shape[0]
    g, d, yy = G[j], np.diag(G), G[j, j]
    w, q = np.zeros(n), np.zeros(n)
    last = np.inf
    for it in range(1, max_iter + 1):
        dmax = wmax = 0.0
        for i in range(n):
            if i == j or not d[i] > 0:
                continue
            old = w[i]
            t = g[i] - (q[i] - d[i] * old) - l1
            new = t / (d[i] + l2) if t > 0 else 0.0
            if new != old:
                row = G[i].copy()
                row[j] = 0
                q += (new - old) * row
                w[i] = new
                if trace is not None:
                    trace.append((it, i))
            dmax, wmax = max(dmax, abs(new - old)), max(wmax, abs(new))
        if wmax == 0 or dmax <= tol * wmax or it == max_iter:
            last = gap(G, j, w, q, l1, l2)
            if (tol > 0 and last <= tol * yy) or (tol == 0 and dmax == 0):
                break
    return w, it, last


def fit(G, l1, l2, tol, max_iter, columns=None):
    """(Wt [n, n] with Wt[j] = w of column j, n_iter [n], gap [n]); columns outside `columns` stay zero."""
    n = G.shape[0]
    Wt, n_iter, gaps = np.zeros((n, n)), np.zeros(n, np.int32), np.zeros(n)
    for j in (range(n) if columns is None else columns):
        Wt[j], n_iter[j], gaps[j] = solve(G, j, l1, l2, tol, max_iter)
    return Wt, n_iter, gaps


def objective(X, j, w, l1, l2):
    """P_j(w) from X itself, not from G."""
    Xz = np.array(X, np.float64)
    y = Xz[:, j].copy()
    Xz[:, j] = 0
    r = y - Xz @ w
    return 0.5 * (r @ r) + l1 * np.abs(w).sum() + 0.5 * l2 * (w @ w)


def golden_matrix():
    """The 60 x 37 matrix of tests/golden/slim_ref.npz: power-law columns, item 5 empty, user 0 holding every other."""
    rng = np.random.RandomState(3)
    U, N = 60, 37
    pop = 1 / np.arange(1, N + 1) ** 0.7
    X = (rng.random_sample((U, N)) < np.minimum(0.9, pop * 0.6)).astype(np.float64)
    X[:, 5] = 0
    X[0, :] = 1
    X[0, 5] = 0
    return X


def power_law_matrix(n_users, n_items, seed):
    """0/1 [n_users, n_items]: power-law item popularity; user 0 holds every item that anybody holds, so that every
    pair of them co-occurs; item 3 is empty (its column has no candidate at any l1) and item 7 is held by user 0
    alone."""
    rng = np.random.RandomState(seed)
    pop = 1 / np.arange(1, n_items + 1) ** 0.7
    X = (rng.random_sample((n_users, n_items)) < np.minimum(0.9, pop * 0.6)).astype(np.float64)
    X[0, :] = 1
    X[:, 3] = 0
    X[1:, 7] = 0
    return X


def score_rows(users, indptr, indices, W):
    """Rows of X @ W for `users`, added in the CSR's stored (ascending) order from 0.0 (scipy's csr @ dense order)."""
    out = np.zeros((len(users), W.shape[1]))
    for q, u in enumerate(users):
        acc = out[q]
        for i in indices[indptr[u]:indptr[u + 1]]:
            acc = acc + W[i]
        out[q] = acc
    return out
