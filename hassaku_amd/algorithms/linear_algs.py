"""EASE and SLIM on the HIP device (algorithms/linear_algs.py of the reference: EASE 131-176, Steck, arXiv:1905.03375;
SLIM 14-128, described at its class below).

EASE.fit(X), X the binary user x item train matrix:
  * X^T is packed into the dense int8 operand of the neighbourhood models (hsk_knn_pack_i8) and the co-occurrence
    counts X^T X come block by block from the int8 matrix cores (hsk_knn_gram_i8, exact int32);
  * hsk_ease_gram_f64 turns a count block into rows of the fp64 G = X^T X + int(lam) I;
  * hsk_ease_inverse_f64 inverts G in place on the fp64 matrix cores (blocked Gauss-Jordan, no pivoting: G is SPD);
  * hsk_ease_weights scales it in place to B = P / (-diag P) with a zero diagonal.
The item x item B is what the model keeps.  The reference's dense users x items `pred_mtx = X @ B` is never built:
score_rows() sums, per user, the rows of B its items pick, in ascending item order from 0.0 -- scipy's csr @ dense
order -- so given the same B a row is bitwise the reference's.
"""
import logging
import math
import os

import numpy as np
import torch

from hassaku_amd import hip_ops
from hassaku_amd.algorithms.base_classes import FittedRecommenderAlgorithm, csr_arrays


def _lam_int(lam) -> int:
    """int(lam) as the reference takes it (linear_algs.py:154), refusing what has no such value or gives less than 1."""
    if isinstance(lam, (bool, np.bool_)) or not isinstance(lam, (int, float, np.integer, np.floating)):
        raise ValueError(f'lam = {lam!r} must be a number')
    if not math.isfinite(lam) or int(lam) < 1:
        raise ValueError(f'lam = {lam!r} must be a finite number with int(lam) >= 1 (G = X^T X alone may be singular)')
    return int(lam)


def validate_ease_conf(conf: dict):
    """The EASE key of a conf (linear_algs.py:176): `lam`, truncated to an integer by the reference's fit.  lam below 1
    (the reference accepts 0 and then inverts a possibly singular G) is refused."""
    if 'lam' not in conf:
        raise ValueError('EASE conf needs lam')
    _lam_int(conf['lam'])


class EASE(FittedRecommenderAlgorithm):
    GRAM_BLOCK_BYTES = 1 << 30   # int32 counts of one row block
    WINDOW = 1024                # item window of one scoring workgroup

    def __init__(self, lam, device='cuda'):
        super().__init__(device)
        self.lam = lam
        self.lam_int = _lam_int(lam)
        self.name = 'EASE'
        self.B = None              # fp64 [n_items, n_items] on the device
        logging.info('Built %s: lam %s (int %d)', self.name, lam, self.lam_int)

    # ------------------------------------------------------------------ fit
    def _gram_block(self, n: int) -> int:
        block = max(128, (self.GRAM_BLOCK_BYTES // (4 * n)) // 128 * 128)
        return min(block, -(-n // 128) * 128)

    def fit_bytes(self, n_users: int, n_items: int) -> int:
        """Device bytes fit() allocates: G, the int8 operand of X^T, one count block and the inverse's panels."""
        rows_pad, k_pad = hip_ops.knn_pack_dims(n_items, n_users)
        return (8 * n_items * n_items + rows_pad * k_pad + 4 * self._gram_block(n_items) * n_items +
                hip_ops.ease_inverse_ws_bytes(n_items))

    def fit(self, matrix):
        indptr, indices, n_users, n_items = csr_arrays(matrix)
        dev = self.device
        self._require_free(self.fit_bytes(n_users, n_items), f'{n_items} items')
        self.B = self.pred_mtx = None     # a fit that raises leaves no model behind, not the old B on a new matrix
        x_ptr, x_idx, t_ptr, t_idx = self._upload(indptr, indices, transpose=(n_users, n_items))
        M = hip_ops.knn_pack_i8(t_ptr, t_idx, n_items, n_users)
        block = self._gram_block(n_items)
        C = torch.empty((block, n_items), dtype=torch.int32, device=dev)
        G = torch.empty((n_items, n_items), dtype=torch.float64, device=dev)
        for r0 in range(0, n_items, block):
            r1 = min(r0 + block, n_items)
            hip_ops.knn_gram_i8(M, n_items, r0, r1, out=C)
            hip_ops.ease_gram_f64(C, r1 - r0, r0, self.lam_int, G)
        del M, C
        hip_ops.ease_inverse_f64(G)       # raises if a pivot was not positive and finite
        self.B = hip_ops.ease_weights(G)
        self.train, self.n_users, self.n_items = (x_ptr, x_idx), n_users, n_items

    def weights(self) -> np.ndarray:
        """B as a numpy array [n_items, n_items]."""
        return self.B.cpu().numpy()

    # ------------------------------------------------------------------ scoring
    def score_rows(self, u_idxs: torch.Tensor, excl=None, out=None) -> torch.Tensor:
        u = u_idxs.to(self.device, torch.int64).contiguous()
        if self.pred_mtx is not None:
            return self._dense_rows(u, excl)
        if self.B is None:
            raise RuntimeError(f'{self.name}: run fit() or load_model_from_path() first')
        return hip_ops.ease_score_rows(u, (*self.train, self.n_users), self.B, window=self.WINDOW, excl=excl, out=out,
                                       status=self._status_word())

    # ------------------------------------------------------------------ persistence
    def save_model_to_path(self, path: str):
        np.savez(os.path.join(path, 'model.npz'), alg=np.array('ease'), lam=np.float64(self.lam),
                 n_users=np.int64(self.n_users), n_items=np.int64(self.n_items), B=self.weights(),
                 train_indptr=self.train[0].cpu().numpy(), train_indices=self.train[1].cpu().numpy())
        logging.info('Model Saved')

    def load_model_from_path(self, path: str):
        with np.load(os.path.join(path, 'model.npz')) as f:
            if 'pred_mtx' in f:       # written by the reference (linear_algs.py:163-166): dense float64 predictions
                self._load_pred_mtx(f)
                self.B = None
            else:
                self._check_alg(f, 'ease')
                n_users, n_items = int(f['n_users']), int(f['n_items'])
                B = f['B']
                if B.shape != (n_items, n_items):
                    raise ValueError(f'B of model.npz has shape {B.shape}, expected ({n_items}, {n_items})')
                train = self._read_train(f, n_users, n_items)
                self.n_users, self.n_items = n_users, n_items
                self.B = torch.from_numpy(np.ascontiguousarray(B, np.float64)).to(self.device)
                self.train = self._upload(*train)
                self.pred_mtx = None
        logging.info('Model Loaded')

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        validate_ease_conf(conf)
        return EASE(conf['lam'])


# ---------------------------------------------------------------------------------------------------------- SLIM
def _number(conf: dict, key: str) -> float:
    v = conf[key]
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f'{key} = {v!r} must be a number')
    return float(v)


def validate_slim_conf(conf: dict):
    """The SLIM keys of a conf (linear_algs.py:128): `alpha` (finite and > 0), `l1_ratio` (a number in [0, 1]) and
    `max_iter` (an integer >= 1), all required; anything else raises ValueError."""
    for key in ('alpha', 'l1_ratio', 'max_iter'):
        if key not in conf:
            raise ValueError(f'SLIM conf needs {key}')
    alpha, l1_ratio = _number(conf, 'alpha'), _number(conf, 'l1_ratio')
    if not (math.isfinite(alpha) and alpha > 0):
        raise ValueError(f"alpha = {conf['alpha']!r} must be finite and > 0")
    if not 0 <= l1_ratio <= 1:       # false for nan
        raise ValueError(f"l1_ratio = {conf['l1_ratio']!r} must be in [0, 1]")
    max_iter = conf['max_iter']
    if isinstance(max_iter, (bool, np.bool_)) or not isinstance(max_iter, (int, np.integer)):
        raise ValueError(f'max_iter = {max_iter!r} must be an integer')
    if max_iter < 1:
        raise ValueError(f'max_iter = {max_iter!r} must be >= 1')


class SLIM(FittedRecommenderAlgorithm):
    """SLIM on the HIP device (algorithms/linear_algs.py:14-128 of the reference; Ning & Karypis, ICDM 2011).

    fit(X): the exact G = X^T X as EASE builds it (int8 matrix cores, nothing added to the diagonal), then
    hsk_slim_cd_f64 solves, per item j, the reference's ElasticNet(positive=True, fit_intercept=False, tol=1e-4) on X
    with column j zeroed by cyclic coordinate descent on G alone (the reference draws coordinates at random: the
    problem and the stop test are its, the iterates are the deterministic law of DESIGN.md section 5.10).  The model
    keeps the dense fp64 item x item W (W[i, j] the weight of item i for target j) and the train CSR; score_rows() is
    EASE's gather-sum, and the reference's dense users x items `pred_mtx = X @ W` is never built."""
    GRAM_BLOCK_BYTES = EASE.GRAM_BLOCK_BYTES
    WINDOW = EASE.WINDOW
    TOL = 1e-4                 # the reference's ElasticNet(tol=...); an instance attribute `tol` overrides it

    def __init__(self, alpha, l1_ratio, max_iter, device='cuda'):
        super().__init__(device)
        validate_slim_conf({'alpha': alpha, 'l1_ratio': l1_ratio, 'max_iter': max_iter})
        self.alpha, self.l1_ratio, self.max_iter = float(alpha), float(l1_ratio), int(max_iter)
        self.tol = self.TOL
        self.name = 'SLIM'
        self.W = None              # fp64 [n_items, n_items] on the device
        self.n_iter_ = self.gap_ = None
        logging.info('Built %s: alpha %s, l1_ratio %s, max_iter %d', self.name, alpha, l1_ratio, self.max_iter)

    # ------------------------------------------------------------------ fit
    _gram_block = EASE._gram_block

    def penalties(self, n_users: int):
        """(l1, l2) of the solver: sklearn's objective times n_users."""
        return n_users * self.alpha * self.l1_ratio, n_users * self.alpha * (1 - self.l1_ratio)

    def fit_bytes(self, n_users: int, n_items: int) -> int:
        """Device bytes fit() allocates: G, Wt and W, the int8 operand of X^T, one count block and the workspace."""
        rows_pad, k_pad = hip_ops.knn_pack_dims(n_items, n_users)
        return (3 * 8 * n_items * n_items + rows_pad * k_pad + 4 * self._gram_block(n_items) * n_items +
                hip_ops.slim_ws_bytes(n_items) + 12 * n_items)

    def fit(self, matrix):
        indptr, indices, n_users, n_items = csr_arrays(matrix)
        dev = self.device
        self._require_free(self.fit_bytes(n_users, n_items), f'{n_items} items')
        self.W = self.pred_mtx = self.n_iter_ = self.gap_ = None     # a fit that raises leaves no model behind
        x_ptr, x_idx, t_ptr, t_idx = self._upload(indptr, indices, transpose=(n_users, n_items))
        M = hip_ops.knn_pack_i8(t_ptr, t_idx, n_items, n_users)
        block = self._gram_block(n_items)
        C = torch.empty((block, n_items), dtype=torch.int32, device=dev)
        G = torch.empty((n_items, n_items), dtype=torch.float64, device=dev)
        for r0 in range(0, n_items, block):
            r1 = min(r0 + block, n_items)
            hip_ops.knn_gram_i8(M, n_items, r0, r1, out=C)
            hip_ops.ease_gram_f64(C, r1 - r0, r0, 0, G)
        del M, C
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        l1, l2 = self.penalties(n_users)
        Wt, n_iter, gap = hip_ops.slim_cd(G, l1, l2, self.tol, self.max_iter, status=status)
        if int(status.item()) & hip_ops.STATUS_NOT_FINITE:
            raise ValueError(f'{self.name}.fit: the solver met a non-finite value (HSK_STATUS_NOT_FINITE)')
        del G
        self.W = Wt.t().contiguous()
        self.n_iter_, self.gap_ = n_iter, gap
        self.train, self.n_users, self.n_items = (x_ptr, x_idx), n_users, n_items

    def weights(self) -> np.ndarray:
        """W as a numpy array [n_items, n_items]."""
        return self.W.cpu().numpy()

    # ------------------------------------------------------------------ scoring
    def score_rows(self, u_idxs: torch.Tensor, excl=None, out=None) -> torch.Tensor:
        if self.pred_mtx is None and self.W is None:
            raise RuntimeError(f'{self.name}: run fit() or load_model_from_path() first')
        u = u_idxs.to(self.device, torch.int64).contiguous()
        if self.pred_mtx is not None:
            return self._dense_rows(u, excl)
        return hip_ops.ease_score_rows(u, (*self.train, self.n_users), self.W, window=self.WINDOW, excl=excl, out=out,
                                       status=self._status_word())

    # ------------------------------------------------------------------ persistence
    def save_model_to_path(self, path: str):
        np.savez(os.path.join(path, 'model.npz'), alg=np.array('slim'), alpha=np.float64(self.alpha),
                 l1_ratio=np.float64(self.l1_ratio), max_iter=np.int64(self.max_iter),
                 n_users=np.int64(self.n_users), n_items=np.int64(self.n_items), W=self.weights(),
                 train_indptr=self.train[0].cpu().numpy(), train_indices=self.train[1].cpu().numpy())
        logging.info('Model Saved')

    def load_model_from_path(self, path: str):
        with np.load(os.path.join(path, 'model.npz')) as f:
            if 'pred_mtx' in f:       # written by the reference (linear_algs.py:115-118): dense float64 predictions
                self._load_pred_mtx(f)
                self.W = None
            else:
                self._check_alg(f, 'slim')
                n_users, n_items = int(f['n_users']), int(f['n_items'])
                W = f['W']
                if W.shape != (n_items, n_items) or W.dtype.kind != 'f':
                    raise ValueError(f'W of model.npz is {W.dtype} {W.shape}, expected floats ({n_items}, {n_items})')
                train = self._read_train(f, n_users, n_items)
                self.n_users, self.n_items = n_users, n_items
                self.W = torch.from_numpy(np.ascontiguousarray(W, np.float64)).to(self.device)
                self.train = self._upload(*train)
                self.pred_mtx = None
            self.n_iter_ = self.gap_ = None
        logging.info('Model Loaded')

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        validate_slim_conf(conf)
        return SLIM(conf['alpha'], conf['l1_ratio'], conf['max_iter'])
