"""numpy-only float64 restatement of implicit-feedback ALS (Hu, Koren, Volinsky) -- the expected values of
tests/test_als.py.  Written from the method, not from any code; the `implicit` package, which the reference calls, is
not consulted.

X is the binary user x item train matrix; a stored entry has confidence alpha and preference 1, every other entry
confidence 1 and preference 0.  One half-sweep solves every row r of a CSR (X for the users, X^T for the items) against
the other side's factors Y (n_other x k):

    G   = Y^T Y
    A_r = G + reg I + (alpha - 1) sum_{i in row r} y_i y_i^T
    b_r = alpha sum_{i in row r} y_i
    x_r = A_r^-1 b_r                    (a row without entries: x_r = 0 exactly, no solve)

One iteration solves the users from the items, then the items from the new users.  The start is
RandomState(seed).random_sample((n_users, k)) * 0.01, then the same call for the items, from one stream.

The bound of one row (row_bound), with u = 2^-53 and gamma_n = n u / (1 - n u):
  * forming A_r and b_r in any summation order perturbs them by at most gamma_m |A|_+ and gamma_deg |b|_+ elementwise,
    m = n_other + deg + 2 (n_other products for G, deg for the row's own sum, the scaling and the shift), with
    |A|_+ = |Y|^T |Y| + reg I + |alpha - 1| |Y_r|^T |Y_r| and |b|_+ = alpha sum |y_i|; in the 2-norm that is at most
    gamma_m || |A|_+ ||_2 and gamma_deg || |b|_+ ||_2;
  * Cholesky and the two triangular solves give (A + dA) x^ = b with ||dA||_2 <= k gamma_{3k+1} (1 - k gamma_{k+1})^-1
    ||A||_2 (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 10.4 and equation 10.7);
  * together (Higham, Theorem 7.2, normwise): ||x^ - x||_2 / ||x||_2 <= kappa_2(A) eps / (1 - kappa_2(A) eps), eps the sum
    of the three relative perturbations.
The tests allow twice that, because numpy's own solve is one such evaluation."""
import numpy as np

SEED = 0
U = 2.0 ** -53


def gamma(n):
    return n * U / (1 - n * U)


# ------------------------------------------------------------------------------------------------------ the method
def init(n_users, n_items, k, seed=SEED):
    rng = np.random.RandomState(seed)
    return rng.random_sample((n_users, k)) * 0.01, rng.random_sample((n_items, k)) * 0.01


def row_system(ids, Y, G, alpha, reg):
    """(A_r, b_r) of the row whose column ids are `ids`."""
    Yr = Y[ids]
    return G + reg * np.eye(Y.shape[1]) + (alpha - 1.0) * (Yr.T @ Yr), alpha * Yr.sum(0)


def half_sweep(csr, Y, alpha, reg, with_bound=False):
    """csr = (indptr, indices) over the rows to solve.  -> X [n_rows, k]; with_bound: (X, row_bound of every row; 0 for a
    row without entries)."""
    indptr, indices = csr
    n, k = len(indptr) - 1, Y.shape[1]
    G = Y.T @ Y
    absG = np.abs(Y).T @ np.abs(Y)
    X, bounds = np.zeros((n, k)), np.zeros(n)
    for r in range(n):
        ids = indices[indptr[r]:indptr[r + 1]]
        if len(ids) == 0:
            continue
        A, b = row_system(ids, Y, G, alpha, reg)
        X[r] = np.linalg.solve(A, b)
        if with_bound:
            aY = np.abs(Y[ids])
            absA = absG + reg * np.eye(k) + abs(alpha - 1.0) * (aY.T @ aY)
            bounds[r] = row_bound(A, absA, b, alpha * aY.sum(0), Y.shape[0] + len(ids) + 2, len(ids))
    return (X, bounds) if with_bound else X


def transpose(csr, n_cols):
    """(indptr, indices) of the transpose, each row's ids ascending."""
    indptr, indices = csr
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    o = np.lexsort((rows, indices))
    t_ptr = np.zeros(n_cols + 1, np.int64)
    np.cumsum(np.bincount(indices, minlength=n_cols), out=t_ptr[1:])
    return t_ptr, rows[o].astype(np.int32)


def fit(csr, n_items, k, alpha, reg, n_iterations, seed=SEED):
    """-> (users_factors, items_factors) after n_iterations x (users from items, items from the new users)."""
    n_users = len(csr[0]) - 1
    Uf, Vf = init(n_users, n_items, k, seed)
    csr_t = transpose(csr, n_items)
    for _ in range(n_iterations):
        Uf = half_sweep(csr, Vf, alpha, reg)
        Vf = half_sweep(csr_t, Uf, alpha, reg)
    return Uf, Vf


def dense(csr, n_cols):
    indptr, indices = csr
    X = np.zeros((len(indptr) - 1, n_cols))
    X[np.repeat(np.arange(len(indptr) - 1), np.diff(indptr)), indices] = 1.0
    return X


def objective(X, Uf, Vf, alpha, reg):
    """sum_ui c_ui (p_ui - u . v)^2 + reg (||U||^2 + ||V||^2), X dense binary, c = 1 + (alpha - 1) X, p = X."""
    R = X - Uf @ Vf.T
    return float(((1.0 + (alpha - 1.0) * X) * R * R).sum() + reg * ((Uf * Uf).sum() + (Vf * Vf).sum()))


# ------------------------------------------------------------------------------------------------------ the bound
def row_bound(A, absA, b, absb, m, deg):
    """The bound on ||x^ - x||_2 / ||x||_2 of the module docstring for one row: A, b the system, absA = |A|_+,
    absb = |b|_+, m = n_other + deg + 2.  inf where kappa_2(A) eps >= 1."""
    k = A.shape[0]
    s = np.linalg.svd(A, compute_uv=False)
    kappa, normA = s[0] / s[-1], s[0]
    eps = (gamma(m) * np.linalg.norm(absA, 2) / normA + gamma(deg) * np.linalg.norm(absb) / np.linalg.norm(b) +
           k * gamma(3 * k + 1) / (1 - k * gamma(k + 1)))
    return kappa * eps / (1 - kappa * eps) if kappa * eps < 1 else np.inf


def row_errors(got, ref):
    """||got_r - ref_r||_2 / ||ref_r||_2 per row (0 where both are exactly 0)."""
    num, den = np.sqrt(((got - ref) ** 2).sum(1)), np.sqrt((ref * ref).sum(1))
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0))
