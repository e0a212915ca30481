"""SVD on the HIP device (algorithms/mf_algs.py:13-65 of the reference, which calls scipy.sparse.linalg.svds).

The leading k = n_factors singular triplets of the binary user x item train matrix X by block subspace iteration with
Rayleigh-Ritz on A = X^T X, which is never formed.  With b = min(round_up(k + OVERSAMPLE, 16),
n_users, n_items) columns:
    V  <- orth(orth(V0))                      V0 = RandomState(SEED).standard_normal((n_items, b)), made on the host
    repeat (at most MAX_ITER times):
        Z = X V,  Y = X^T Z                   hsk_svd_spmm_f64 on the CSR of X and of X^T
        H = Z^T Z (= V^T A V)                 hsk_svd_gram_f64; symmetrised, eigh on the host, theta descending
        V' = V Q,  Y' = Y Q                   hsk_svd_mul_f64
        r_j = || Y'[:, j] - theta_j V'[:, j] ||      hsk_svd_residuals_f64
        stop when max_{j < k} r_j <= TOL theta_1
        V  <- orth(orth(Y'))
    items_factors = V'[:, :k],  users_factors = X items_factors (= U S),  singular_values = sqrt(theta[:k])
orth(Y) normalises the columns (zero columns are dropped), takes the Gram M = Y^T Y on the device and eigh(M) on the
host, drops the directions with w <= width 2^-52 w_max and returns Y (Q_kept / sqrt(w_kept)): no Cholesky, no pivot to
fail, and a block that shrinks when X has fewer independent directions than b.  The host's share is b x b.
The reference's dense users x items product is never built: score_rows() multiplies the factor rows on the fp64
matrix cores.  svds' ascending column order and its signs are not reproduced; the product of the factors is what the
two share."""
import logging

import numpy as np
import torch

from hassaku_amd import hip_ops
from hassaku_amd.algorithms.base_classes import FactorAlgorithm, csr_arrays
from hassaku_amd.conf import checks


def validate_svd_conf(conf: dict):
    """The SVD key of a conf (mf_algs.py:65): `n_factors`, required as the reference's build_from_conf does."""
    checks.require(conf, 'SVDAlgorithm', 'n_factors')
    checks.integer('n_factors', conf['n_factors'], 1)


class SVDAlgorithm(FactorAlgorithm):
    ALG, WIDTH, MAX_K = 'svd', 'n_factors', hip_ops.SVD_MAX_BLOCK
    OVERSAMPLE = 32              # columns of the block beyond n_factors (before rounding up to 16)
    TOL = 1e-11                  # residual of the n_factors leading Ritz pairs, relative to theta_1
    MAX_ITER = 1000
    SEED = 0                     # of the host-made start block
    validate_conf = staticmethod(validate_svd_conf)

    def __init__(self, n_factors=100, device='cuda'):
        super().__init__(device)
        self.n_factors = checks.integer('n_factors', n_factors, 1)
        self.name = 'SVDAlgorithm'
        logging.info('Built %s: n_factors %d', self.name, self.n_factors)

    # ------------------------------------------------------------------ fit
    def block_width(self, n_users: int, n_items: int) -> int:
        return min(-(-(self.n_factors + self.OVERSAMPLE) // 16) * 16, n_users, n_items)

    def fit_bytes(self, n_users: int, n_items: int) -> int:
        """Device bytes fit() allocates: Z [n_users, b], three [n_items, b] blocks and the Gram workspace."""
        b = hip_ops.svd_ld(self.block_width(n_users, n_items))
        return (n_users + 3 * n_items) * b * 8 + self._gram_ws_bytes(n_users, n_items, b)

    @staticmethod
    def _gram_ws_bytes(n_users: int, n_items: int, b: int) -> int:
        """The Gram workspace that serves Z and the item blocks at every width the block may shrink to (a narrower
        block has fewer tiles and so more row splits: its workspace is not always the smaller one)."""
        return max(hip_ops.svd_gram_ws_bytes(n, w) for n in (n_users, n_items) for w in range(1, b + 1))

    def _forget(self):
        super()._forget()             # users_factors = U S
        self.singular_values = None   # numpy float64 [k], descending (None for a model loaded from the reference)
        self.n_iter_ = self.residual_ = None

    def hyper(self) -> dict:
        return dict(n_factors=np.int64(self.n_factors), singular_values=self.singular_values)

    def _orth(self, Y, scratch, out, ws):
        """orth(Y) into the leading columns of `out`, the normalised block in `scratch` (both [n, >= width])."""
        dev, width = Y.device, Y.shape[1]
        norms = hip_ops.svd_residuals(Y, Y, torch.zeros(width, dtype=torch.float64, device=dev)).cpu().numpy()
        keep = np.flatnonzero(norms > 0)
        D = np.zeros((width, hip_ops.svd_ld(len(keep))))
        D[keep, np.arange(len(keep))] = 1.0 / norms[keep]
        Yn = hip_ops.svd_mul(Y, torch.from_numpy(D).to(dev)[:, :len(keep)], out=scratch[:, :len(keep)])
        M = hip_ops.svd_gram(Yn, ws=ws).cpu().numpy()
        w, Q = np.linalg.eigh((M + M.T) / 2)
        good = w > len(keep) * 2.0 ** -52 * w.max()
        R = np.zeros((len(keep), hip_ops.svd_ld(int(good.sum()))))
        R[:, :int(good.sum())] = Q[:, good] / np.sqrt(w[good])
        return hip_ops.svd_mul(Yn, torch.from_numpy(R).to(dev)[:, :int(good.sum())], out=out[:, :int(good.sum())])

    def fit(self, matrix):
        indptr, indices, n_users, n_items = csr_arrays(matrix)
        k, dev = self.n_factors, self.device
        if not 1 <= k < min(n_users, n_items):     # what svds demands of k
            raise ValueError(f'n_factors = {k} must be in [1, min(n_users, n_items) = {min(n_users, n_items)})')
        b = self.block_width(n_users, n_items)
        if b > hip_ops.SVD_MAX_BLOCK:
            raise ValueError(f'n_factors = {k} gives a block of {b} columns, at most {hip_ops.SVD_MAX_BLOCK}')
        self._require_free(self.fit_bytes(n_users, n_items), f'{n_users} users x {n_items} items')
        self._forget()                     # a fit that raises leaves no model behind
        x_ptr, x_idx, t_ptr, t_idx = self._upload(indptr, indices, transpose=(n_users, n_items))
        X, Xt = (x_ptr, x_idx, n_items), (t_ptr, t_idx, n_users)
        ld = hip_ops.svd_ld(b)
        Zbuf = torch.empty((n_users, ld), dtype=torch.float64, device=dev)
        P, S, T = (torch.empty((n_items, ld), dtype=torch.float64, device=dev) for _ in range(3))
        ws = torch.empty(self._gram_ws_bytes(n_users, n_items, ld) // 8, dtype=torch.float64, device=dev)
        V0 = np.zeros((n_items, ld))
        V0[:, :b] = np.random.RandomState(self.SEED).standard_normal((n_items, b))
        S.copy_(torch.from_numpy(V0))
        V = self._orth(self._orth(S[:, :b], T, P, ws), T, S, ws)      # V lives in S; P and T are free
        for it in range(1, self.MAX_ITER + 1):
            bc = V.shape[1]
            if bc < k:
                raise ValueError(f'the train matrix has rank {bc} < n_factors = {k}')
            Z = hip_ops.svd_spmm(X, V, out=Zbuf[:, :bc])
            Y = hip_ops.svd_spmm(Xt, Z, out=P[:, :bc])
            H = hip_ops.svd_gram(Z, ws=ws).cpu().numpy()
            theta, Q = np.linalg.eigh((H + H.T) / 2)
            theta = np.ascontiguousarray(theta[::-1])
            Qd = torch.zeros((bc, hip_ops.svd_ld(bc)), dtype=torch.float64)
            Qd[:, :bc] = torch.from_numpy(np.ascontiguousarray(Q[:, ::-1]))
            Qd = Qd.to(dev)[:, :bc]
            Vr = hip_ops.svd_mul(V, Qd, out=T[:, :bc])                # V' in T
            Yr = hip_ops.svd_mul(Y, Qd, out=S[:, :bc])                # Y' in S (V is done with)
            res = hip_ops.svd_residuals(Yr, Vr, torch.from_numpy(theta).to(dev)).cpu().numpy()
            residual = float(res[:k].max())
            if residual <= self.TOL * theta[0]:
                break
            V = self._orth(self._orth(Yr, P, T, ws), P, S, ws)        # back in S; P and T are free
        else:
            raise RuntimeError(f'{self.name}.fit: no convergence in {self.MAX_ITER} iterations: residual '
                               f'{residual:.3e} > {self.TOL * theta[0]:.3e}')
        items = hip_ops.svd_empty(n_items, k, dev)
        items.copy_(Vr[:, :k])
        self.users_factors = hip_ops.svd_spmm(X, items)
        self.items_factors = items
        self.singular_values = np.sqrt(np.maximum(theta[:k], 0.0))
        self.n_users, self.n_items = n_users, n_items
        self.n_iter_, self.residual_ = it, residual

    # ------------------------------------------------------------------ persistence
    def _load_own(self, f, k: int):
        if 'singular_values' in f:
            sv = np.asarray(f['singular_values'], np.float64)
            if sv.shape != (k,):
                raise ValueError(f'singular_values of model.npz has shape {sv.shape}, expected ({k},)')
            self.singular_values = sv

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        validate_svd_conf(conf)
        return SVDAlgorithm(conf['n_factors'])


# ---------------------------------------------------------------------------------------------------------------
# ALS
# ---------------------------------------------------------------------------------------------------------------
def validate_als_conf(conf: dict):
    """The ALS keys of a conf (mf_algs.py:139-142): `alpha`, `factors`, `regularization`, `n_iterations`, required as
    the reference's build_from_conf indexes them; `use_gpu` is optional, a bool, and changes nothing.
    regularization = 0, which the reference takes (and may then invert a singular matrix), is refused."""
    checks.require(conf, 'AlternatingLeastSquare', 'alpha', 'factors', 'regularization', 'n_iterations')
    checks.positive('alpha', conf['alpha'])
    checks.integer('factors', conf['factors'], 1, hip_ops.ALS_MAX_FACTORS)
    checks.positive('regularization', conf['regularization'])
    checks.integer('n_iterations', conf['n_iterations'], 1)
    if 'use_gpu' in conf and not isinstance(conf['use_gpu'], (bool, np.bool_)):
        raise ValueError(f"use_gpu = {conf['use_gpu']!r} must be a bool")


class AlternatingLeastSquare(FactorAlgorithm):
    """Implicit-feedback ALS (Hu, Koren, Volinsky; mf_algs.py:68-142 of the reference, which calls the `implicit`
    package) on the HIP device, DESIGN.md section 5.9.  X is the binary train matrix, a stored entry has confidence
    alpha and preference 1, every other entry confidence 1 and preference 0.  One half-sweep solves every row r of a
    CSR (X for the users, X^T for the items) against the other side's factors Y:
        G = Y^T Y                                                              hsk_svd_gram_f64
        A_r = G + regularization I + (alpha - 1) sum_{i in row r} y_i y_i^T
        b_r = alpha sum_{i in row r} y_i,   x_r = A_r^-1 b_r                   hsk_als_solve_f64 (Cholesky, fp64)
    and a row without entries is exactly 0.  One iteration solves the users from the items, then the items from the
    new users.  The start is RandomState(SEED).random_sample((n_users, k)) * 0.01, then the same call for the items,
    made on the host: `implicit`'s CPU law, not its random stream; its default three conjugate-gradient steps are not
    reproduced (this is its use_cg=False)."""
    ALG, WIDTH, MAX_K = 'als', 'factors', hip_ops.ALS_MAX_FACTORS
    SEED = 0
    validate_conf = staticmethod(validate_als_conf)

    def __init__(self, alpha, factors, regularization, n_iterations, use_gpu=True, device='cuda'):
        super().__init__(device)
        validate_als_conf(dict(alpha=alpha, factors=factors, regularization=regularization, n_iterations=n_iterations,
                               use_gpu=use_gpu))
        self.alpha, self.factors = float(alpha), int(factors)
        self.regularization, self.n_iterations = float(regularization), int(n_iterations)
        self.use_gpu = bool(use_gpu)      # the reference's flag; the fit runs on the device whatever it says
        self.name = 'AlternatingLeastSquare'
        logging.info('Built %s: alpha %g, factors %d, regularization %g, n_iterations %d', self.name, self.alpha,
                     self.factors, self.regularization, self.n_iterations)

    # ------------------------------------------------------------------ fit
    def fit_bytes(self, n_users: int, n_items: int, nnz: int) -> int:
        """Device bytes fit() needs at its peak: both factor blocks, the two issue orders, the Gram workspace and the
        k x k Gram (one for the whole fit), the CSR of X and of X^T (int64 row pointers, int32 ids), and, while the
        transpose is made, csr_transpose's temporaries -- five int64 arrays of nnz entries (the row of every entry, the
        widened ids, the sort key, the permutation and the permuted rows) and an int64 count per item; the sort's own
        scratch is not known here and not counted."""
        ld, k = hip_ops.svd_ld(self.factors), self.factors
        own = (n_users + n_items) * (ld * 8 + 4) + self._gram_ws_bytes(n_users, n_items) + k * k * 8
        csr = (n_users + 1 + n_items + 1) * 8 + 2 * nnz * 4
        return own + csr + 5 * nnz * 8 + n_items * 8

    def _gram_ws_bytes(self, n_users: int, n_items: int) -> int:
        return max(hip_ops.svd_gram_ws_bytes(n, self.factors) for n in (n_users, n_items))

    def hyper(self) -> dict:
        return dict(alpha=np.float64(self.alpha), factors=np.int64(self.factors),
                    regularization=np.float64(self.regularization), n_iterations=np.int64(self.n_iterations))

    @classmethod
    def init_factors(cls, n_users: int, n_items: int, k: int):
        """The host-made start: users first, then items, from one stream."""
        rng = np.random.RandomState(cls.SEED)
        return rng.random_sample((n_users, k)) * 0.01, rng.random_sample((n_items, k)) * 0.01

    def fit(self, matrix):
        indptr, indices, n_users, n_items = csr_arrays(matrix)
        k, dev = self.factors, self.device
        self._forget()                     # a fit that raises, for whatever reason, leaves no model behind
        self._require_free(self.fit_bytes(n_users, n_items, len(indices)),
                           f'{n_users} users x {n_items} items, {len(indices)} entries')
        x_ptr, x_idx, t_ptr, t_idx = self._upload(indptr, indices, transpose=(n_users, n_items))
        X, Xt = (x_ptr, x_idx, n_items), (t_ptr, t_idx, n_users)
        # the longest rows are issued first: one popular item is a whole workgroup's tail
        u_order = torch.from_numpy(np.argsort(-np.diff(indptr), kind='stable').astype(np.int32)).to(dev)
        i_order = torch.from_numpy(np.argsort(-np.bincount(indices, minlength=n_items),
                                              kind='stable').astype(np.int32)).to(dev)
        u0, v0 = self.init_factors(n_users, n_items, k)
        U, V = self._padded(u0), self._padded(v0)
        ws = torch.empty(max(self._gram_ws_bytes(n_users, n_items) // 8, 2), dtype=torch.float64, device=dev)
        G = torch.empty((k, k), dtype=torch.float64, device=dev)      # launches are stream-ordered: one G serves both sides
        status = hip_ops.new_status(dev)
        for _ in range(self.n_iterations):
            hip_ops.als_solve(X, V, hip_ops.svd_gram(V, ws=ws, out=G), self.alpha, self.regularization, order=u_order,
                              out=U, status=status)
            hip_ops.als_solve(Xt, U, hip_ops.svd_gram(U, ws=ws, out=G), self.alpha, self.regularization,
                              order=i_order, out=V, status=status)
        word = int(status.item())
        if word:
            bits = [name for bit, name in ((1, 'HSK_STATUS_BAD_INDEX'), (8, 'HSK_STATUS_NOT_SPD')) if word & bit]
            raise ValueError(f'{self.name}.fit: the solver raised status {word} ({", ".join(bits) or "unknown"}): '
                             f'the train matrix or the factors are not what the law assumes')
        self.users_factors, self.items_factors = U, V
        self.n_users, self.n_items = n_users, n_items

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        validate_als_conf(conf)
        return AlternatingLeastSquare(conf['alpha'], conf['factors'], conf['regularization'], conf['n_iterations'],
                                      conf.get('use_gpu', True))
