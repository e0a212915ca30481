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
import os

import numpy as np
import torch

from hassaku_amd import hip_ops
from hassaku_amd.algorithms.base_classes import FittedRecommenderAlgorithm, csr_arrays


def _n_factors(n_factors) -> int:
    """n_factors as an int, refusing bools, non-integers and values below 1."""
    if isinstance(n_factors, (bool, np.bool_)) or not isinstance(n_factors, (int, np.integer)):
        raise ValueError(f'n_factors = {n_factors!r} must be an integer')
    if n_factors < 1:
        raise ValueError(f'n_factors = {n_factors!r} must be >= 1')
    return int(n_factors)


def validate_svd_conf(conf: dict):
    """The SVD key of a conf (mf_algs.py:65): `n_factors`, required as the reference's build_from_conf does."""
    if 'n_factors' not in conf:
        raise ValueError('SVDAlgorithm conf needs n_factors')
    _n_factors(conf['n_factors'])


class SVDAlgorithm(FittedRecommenderAlgorithm):
    OVERSAMPLE = 32              # columns of the block beyond n_factors (before rounding up to 16)
    TOL = 1e-11                  # residual of the n_factors leading Ritz pairs, relative to theta_1
    MAX_ITER = 1000
    SEED = 0                     # of the host-made start block

    def __init__(self, n_factors=100, device='cuda'):
        super().__init__(device)          # pred_mtx and train stay None: the factors are all a model or a file holds
        self.n_factors = _n_factors(n_factors)
        self.name = 'SVDAlgorithm'
        self.users_factors = None     # fp64 [n_users, k] on the device (= U S); a view of an even-stride buffer
        self.items_factors = None     # fp64 [n_items, k]
        self.singular_values = None   # numpy float64 [k], descending (None for a model loaded from the reference)
        self.n_iter_ = self.residual_ = None
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
        self.users_factors = self.items_factors = self.singular_values = None
        self.n_iter_ = self.residual_ = None

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

    # ------------------------------------------------------------------ scoring
    def score_rows(self, u_idxs: torch.Tensor, excl=None, out=None) -> torch.Tensor:
        if self.items_factors is None:
            raise RuntimeError(f'{self.name}: run fit() or load_model_from_path() first')
        u = u_idxs.to(self.device, torch.int64).contiguous()
        return hip_ops.svd_score_rows(u, self.users_factors, self.items_factors, excl=excl, out=out,
                                      status=self._status_word())

    # ------------------------------------------------------------------ persistence
    def save_model_to_path(self, path: str):
        """The reference's two keys (mf_algs.py:51-54) plus alg, n_factors and singular_values, which its loader
        ignores."""
        np.savez(os.path.join(path, 'model.npz'), users_factors=self.users_factors.cpu().numpy(),
                 items_factors=self.items_factors.cpu().numpy(), alg=np.array('svd'),
                 n_factors=np.int64(self.n_factors), singular_values=self.singular_values)
        logging.info('Model Saved')

    def load_model_from_path(self, path: str):
        """Reads a file written here or by the reference (no `alg` key; float32 if its svds ran on the float32 cast of
        an integer matrix -- any float dtype is taken and held as float64)."""
        with np.load(os.path.join(path, 'model.npz')) as f:       # never with allow_pickle
            uf, vf, k = _read_factors(f, 'svd', self.name, hip_ops.SVD_MAX_BLOCK)
            if 'n_factors' in f and int(f['n_factors']) != k:
                raise ValueError(f"n_factors = {int(f['n_factors'])} of model.npz, but the factors have {k} columns")
            sv = None
            if 'singular_values' in f:
                sv = np.asarray(f['singular_values'], np.float64)
                if sv.shape != (k,):
                    raise ValueError(f'singular_values of model.npz has shape {sv.shape}, expected ({k},)')
        self._forget()
        self.n_factors, self.singular_values = k, sv
        self.n_users, self.n_items = uf.shape[0], vf.shape[0]
        self.users_factors, self.items_factors = self._padded(uf), self._padded(vf)
        logging.info('Model Loaded')

    def _padded(self, a: np.ndarray) -> torch.Tensor:
        return _padded(a, self.device)

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        validate_svd_conf(conf)
        return SVDAlgorithm(conf['n_factors'])


# ---------------------------------------------------------------------------------------------------------------
# what the two factor models share: the two keys of the reference's model.npz and the padded device layout
# ---------------------------------------------------------------------------------------------------------------
def _read_factors(f, alg: str, name: str, max_k: int):
    """(users_factors, items_factors, k) of an open model.npz written here (`alg` must match) or by the reference (no
    `alg` key; any float dtype), validated: two 2-D float arrays that share a number of factors in [1, max_k]."""
    if 'alg' in f and str(f['alg']) != alg:
        raise ValueError(f"model.npz holds a {str(f['alg'])} model, not {name}")
    for key in ('users_factors', 'items_factors'):
        if key not in f:
            raise ValueError(f'model.npz has no {key}')
    try:
        uf, vf = f['users_factors'], f['items_factors']
    except ValueError as e:
        raise ValueError('the factors of model.npz are object arrays; they are not unpickled') from e
    for key, a in (('users_factors', uf), ('items_factors', vf)):
        if a.ndim != 2 or not np.issubdtype(a.dtype, np.floating):
            raise ValueError(f'{key} of model.npz must be a 2-D float array, got {a.dtype} {a.shape}')
    k = uf.shape[1]
    if vf.shape[1] != k or not 1 <= k <= max_k or uf.shape[0] < 1 or vf.shape[0] < 1:
        raise ValueError(f'users_factors {uf.shape} and items_factors {vf.shape} of model.npz do not share a '
                         f'number of factors in [1, {max_k}]')
    return uf, vf, k


def _padded(a: np.ndarray, device) -> torch.Tensor:
    """[n, k] float64 on the device as a view of an even-stride buffer (16-byte aligned rows for any k)."""
    buf = np.zeros((a.shape[0], hip_ops.svd_ld(a.shape[1])), np.float64)
    buf[:, :a.shape[1]] = a
    return torch.from_numpy(buf).to(device)[:, :a.shape[1]]


# ---------------------------------------------------------------------------------------------------------------
# ALS
# ---------------------------------------------------------------------------------------------------------------
def _als_int(conf_key: str, v, lo: int, hi=None) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError(f'{conf_key} = {v!r} must be an integer')
    if v < lo or (hi is not None and v > hi):
        raise ValueError(f'{conf_key} = {v!r} must be in [{lo}, {hi}]' if hi is not None else
                         f'{conf_key} = {v!r} must be >= {lo}')
    return int(v)


def _als_positive(conf_key: str, v) -> float:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f'{conf_key} = {v!r} must be a number')
    if not (np.isfinite(v) and v > 0):
        raise ValueError(f'{conf_key} = {v!r} must be finite and > 0')
    return float(v)


def validate_als_conf(conf: dict):
    """The ALS keys of a conf (mf_algs.py:139-142): `alpha`, `factors`, `regularization`, `n_iterations`, required as
    the reference's build_from_conf indexes them; `use_gpu` is optional, a bool, and changes nothing.
    regularization = 0, which the reference takes (and may then invert a singular matrix), is refused."""
    for key in ('alpha', 'factors', 'regularization', 'n_iterations'):
        if key not in conf:
            raise ValueError(f'AlternatingLeastSquare conf needs {key}')
    _als_positive('alpha', conf['alpha'])
    _als_int('factors', conf['factors'], 1, hip_ops.ALS_MAX_FACTORS)
    _als_positive('regularization', conf['regularization'])
    _als_int('n_iterations', conf['n_iterations'], 1)
    if 'use_gpu' in conf and not isinstance(conf['use_gpu'], (bool, np.bool_)):
        raise ValueError(f"use_gpu = {conf['use_gpu']!r} must be a bool")


class AlternatingLeastSquare(FittedRecommenderAlgorithm):
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
    SEED = 0

    def __init__(self, alpha, factors, regularization, n_iterations, use_gpu=True, device='cuda'):
        super().__init__(device)
        self.alpha = _als_positive('alpha', alpha)
        self.factors = _als_int('factors', factors, 1, hip_ops.ALS_MAX_FACTORS)
        self.regularization = _als_positive('regularization', regularization)
        self.n_iterations = _als_int('n_iterations', n_iterations, 1)
        if not isinstance(use_gpu, (bool, np.bool_)):
            raise ValueError(f'use_gpu = {use_gpu!r} must be a bool')
        self.use_gpu = bool(use_gpu)      # the reference's flag; the fit runs on the device whatever it says
        self.name = 'AlternatingLeastSquare'
        self.users_factors = None     # fp64 [n_users, k] on the device; a view of an even-stride buffer
        self.items_factors = None     # fp64 [n_items, k]
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

    def _forget(self):
        self.users_factors = self.items_factors = None

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
        U, V = _padded(u0, dev), _padded(v0, dev)
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

    # ------------------------------------------------------------------ scoring
    def score_rows(self, u_idxs: torch.Tensor, excl=None, out=None) -> torch.Tensor:
        if self.items_factors is None:
            raise RuntimeError(f'{self.name}: run fit() or load_model_from_path() first')
        u = u_idxs.to(self.device, torch.int64).contiguous()
        return hip_ops.svd_score_rows(u, self.users_factors, self.items_factors, excl=excl, out=out,
                                      status=self._status_word())

    # ------------------------------------------------------------------ persistence
    def save_model_to_path(self, path: str):
        """The reference's two keys (mf_algs.py:127-130) plus alg and the hyper-parameters, which its loader ignores."""
        np.savez(os.path.join(path, 'model.npz'), users_factors=self.users_factors.cpu().numpy(),
                 items_factors=self.items_factors.cpu().numpy(), alg=np.array('als'), alpha=np.float64(self.alpha),
                 factors=np.int64(self.factors), regularization=np.float64(self.regularization),
                 n_iterations=np.int64(self.n_iterations))
        logging.info('Model Saved')

    def load_model_from_path(self, path: str):
        """Reads a file written here or by the reference (no `alg` key; `implicit` returns float32 factors -- any float
        dtype is taken and held as float64)."""
        with np.load(os.path.join(path, 'model.npz')) as f:       # never with allow_pickle
            uf, vf, k = _read_factors(f, 'als', self.name, hip_ops.ALS_MAX_FACTORS)
            if 'factors' in f and int(f['factors']) != k:
                raise ValueError(f"factors = {int(f['factors'])} of model.npz, but the factors have {k} columns")
        self._forget()
        self.factors = k
        self.n_users, self.n_items = uf.shape[0], vf.shape[0]
        self.users_factors, self.items_factors = _padded(uf, self.device), _padded(vf, self.device)
        logging.info('Model Loaded')

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        validate_als_conf(conf)
        return AlternatingLeastSquare(conf['alpha'], conf['factors'], conf['regularization'], conf['n_iterations'],
                                      conf.get('use_gpu', True))
