"""numpy-only float64 restatement of the SVD model -- the expected values of tests/test_svd.py, which holds it to the
g14 goldens (written by the reference's scipy.sparse.linalg.svds) on the CPU.  Written from the method, not from any
code:

block subspace iteration with Rayleigh-Ritz on A = X^T X (never formed), X the binary n_users x n_items train matrix,
k = n_factors, block width b = min(round_up(k + OVERSAMPLE, 16), n_users, n_items):

    V  <- orth(orth(V0))                      V0 = RandomState(SEED).standard_normal((n_items, b))
    repeat (at most MAX_ITER times):
        Z = X V,  Y = X^T Z,  H = Z^T Z (= V^T A V, symmetrised),  theta, Q = eigh(H), theta descending
        V' = V Q,  Y' = Y Q,  r_j = || Y'[:, j] - theta_j V'[:, j] ||
        stop when max_{j < k} r_j <= TOL theta_1
        V  <- orth(orth(Y'))
    items_factors = V'[:, :k],  users_factors = X items_factors (= U S),  singular_values = sqrt(theta[:k])

orth(Y) normalises the columns (zero columns are dropped), takes M = Y^T Y, eigh(M) and drops the directions with
w <= width 2^-52 w_max; the result is Y (Q_kept / sqrt(w_kept)).  Also each device kernel's contract in numpy, and the
bounds the tests use (u = 2^-53, gamma_n = n u / (1 - n u))."""
import numpy as np
import scipy.sparse as sp

OVERSAMPLE, TOL, MAX_ITER, SEED = 32, 1e-11, 1000, 0
U = 2.0 ** -53


# ------------------------------------------------------------------------------------------------------ the method
def block_width(k, n_users, n_items):
    return min(-(-(k + OVERSAMPLE) // 16) * 16, n_users, n_items)


def start_block(n_items, b):
    return np.random.RandomState(SEED).standard_normal((n_items, b))


def csr(indptr, indices, n_rows, n_cols):
    """The binary matrix as a scipy CSR of float64 ones (stored order kept)."""
    return sp.csr_matrix((np.ones(len(indices)), np.asarray(indices), np.asarray(indptr)), shape=(n_rows, n_cols))


def orth(Y):
    norms = np.sqrt((Y * Y).sum(0))
    keep = norms > 0
    Y = Y[:, keep] * (1.0 / norms[keep])
    M = Y.T @ Y
    w, Q = np.linalg.eigh((M + M.T) / 2)
    good = w > Y.shape[1] * 2.0 ** -52 * w.max()
    return Y @ (Q[:, good] / np.sqrt(w[good]))


def fit(X, k, max_iter=MAX_ITER):
    """X: scipy CSR of ones.  -> dict(items_factors, users_factors, singular_values, n_iter, residual, V) with V the
    whole final block V'."""
    n_users, n_items = X.shape
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= k < min(n_users, n_items):
        raise ValueError(f'n_factors = {k!r} must be an integer in [1, min(n_users, n_items) = {min(X.shape)})')
    Xt = X.T.tocsr()
    Xt.sort_indices()
    V = orth(orth(start_block(n_items, block_width(k, n_users, n_items))))
    for it in range(1, max_iter + 1):
        if V.shape[1] < k:
            raise ValueError(f'the train matrix has rank {V.shape[1]} < n_factors = {k}')
        Z = X @ V
        Y = Xt @ Z
        H = Z.T @ Z
        theta, Q = np.linalg.eigh((H + H.T) / 2)
        theta, Q = theta[::-1].copy(), Q[:, ::-1].copy()
        V, Y = V @ Q, Y @ Q
        res = np.sqrt(((Y - theta * V) ** 2).sum(0))
        residual = float(res[:k].max())
        if residual <= TOL * theta[0]:
            items = np.ascontiguousarray(V[:, :k])
            return dict(items_factors=items, users_factors=X @ items, n_iter=it, residual=residual, V=V,
                        singular_values=np.sqrt(np.maximum(theta[:k], 0.0)))
        V = orth(orth(Y))
    raise RuntimeError(f'no convergence in {max_iter} iterations: residual {residual:.3e} > {TOL * theta[0]:.3e}')


# ------------------------------------------------------------------------------------------------------ the kernels
def spmm(indptr, indices, V):
    """out[r] = ((0.0 + V[i1]) + V[i2]) + ... over the ids of CSR row r in stored order."""
    out = np.zeros((len(indptr) - 1, V.shape[1]))
    for r in range(len(indptr) - 1):
        acc = out[r]
        for i in indices[indptr[r]:indptr[r + 1]]:
            acc = acc + V[i]
        out[r] = acc
    return out


def gram(A, B):
    return A.T @ B


def mul(A, Q):
    return A @ Q


def residual_squares(Y, V, theta):
    """The sums of squares under the root of the residual kernel."""
    return ((Y - theta * V) ** 2).sum(0)


def score_rows(users, UF, IF, excl=None):
    """UF[users] @ IF^T; excl = (indptr, indices) over user ids -> those columns -inf."""
    out = UF[users] @ IF.T
    if excl is not None:
        for q, u in enumerate(users):
            out[q, excl[1][excl[0][u]:excl[0][u + 1]]] = -np.inf
    return out


# ------------------------------------------------------------------------------------------------------ the bounds
def gamma(n):
    return n * U / (1 - n * U)


def spectrum(X_dense):
    """Singular values of the dense X (descending) from numpy.linalg.svd, and the eigenvalues lambda = sigma^2."""
    s = np.linalg.svd(X_dense, compute_uv=False)
    return s, s * s


def sv_bound(s, k):
    """|sigma_j - reference| <= 2 TOL sigma_1^2 / sigma_k: a Ritz value of A is within the residual TOL lambda_1 of an
    eigenvalue, and d sigma = d lambda / (2 sigma); the factor 2 on top covers the reference's own error."""
    return 2 * TOL * s[0] ** 2 / s[k - 1]


def pred_bound(deg, s, k, gap=None):
    """bound_u = 2 sqrt(deg_u k) TOL lambda_1 / gap, gap = lambda_k - lambda_{k+1}: the Davis-Kahan sin Theta bound on
    the rank-k projector (Frobenius, residual norm <= sqrt(k) TOL lambda_1) times the row norm sqrt(deg_u) of a binary
    row; the factor 2 covers the reference's own error and rounding."""
    lam = s * s
    gap = lam[k - 1] - lam[k] if gap is None else gap
    return 2 * np.sqrt(np.asarray(deg, np.float64) * k) * TOL * lam[0] / gap


def truncated(X_dense, k):
    """numpy.linalg.svd's rank-k product U_k S_k V_k^T."""
    u, s, vt = np.linalg.svd(X_dense, full_matrices=False)
    return (u[:, :k] * s[:k]) @ vt[:k]
