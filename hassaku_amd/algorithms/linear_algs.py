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

import numpy as np
import torch

from hassaku_amd import hip_ops
from hassaku_amd.algorithms.base_classes import ItemWeightAlgorithm, csr_arrays
from hassaku_amd.conf import checks


def _lam_int(lam) -> int:
    """int(lam) as the reference takes it (linear_algs.py:154), refusing what has no such value or gives less than 1."""
    if not math.isfinite(checks.number('lam', lam)) or int(lam) < 1:
        raise ValueError(f'lam = {lam!r} must be a finite number with int(lam) >= 1 (G = X^T X alone may be singular)')
    return int(lam)


def validate_ease_conf(conf: dict):
    """The EASE key of a conf (linear_algs.py:176): `lam`, truncated to an integer by the reference's fit.  lam below 1
    (the reference accepts 0 and then inverts a possibly singular G) is refused."""
    checks.require(conf, 'EASE', 'lam')
    _lam_int(conf['lam'])


class EASE(ItemWeightAlgorithm):
    ALG, WEIGHTS = 'ease', 'B'
    validate_conf = staticmethod(validate_ease_conf)

    def __init__(self, lam, device='cuda'):
        super().__init__(device)
        self.lam = lam
        self.lam_int = _lam_int(lam)
        self.name = 'EASE'
        logging.info('Built %s: lam %s (int %d)', self.name, lam, self.lam_int)

    def hyper(self) -> dict:
        return dict(lam=np.float64(self.lam))

    # ------------------------------------------------------------------ fit
    def fit_bytes(self, n_users: int, n_items: int) -> int:
        """Device bytes fit() allocates: G, the int8 operand of X^T, one count block and the inverse's panels."""
        rows_pad, k_pad = hip_ops.knn_pack_dims(n_items, n_users)
        return (8 * n_items * n_items + rows_pad * k_pad + 4 * self._gram_block(n_items) * n_items +
                hip_ops.ease_inverse_ws_bytes(n_items))

    @staticmethod
    def _inverse(G):
        """G^-1 in place; raises if a pivot was not positive and finite."""
        return hip_ops.ease_inverse_f64(G)

    @staticmethod
    def _weights(P):
        return hip_ops.ease_weights(P)

    def fit(self, matrix):
        indptr, indices, n_users, n_items = csr_arrays(matrix)
        self._require_free(self.fit_bytes(n_users, n_items), f'{n_items} items')
        self._forget()                    # a fit that raises leaves no model behind, not the old B on a new matrix
        G, train = self._gram(indptr, indices, n_users, n_items, self.lam_int)
        self.B = self._weights(self._inverse(G))
        self.train, self.n_users, self.n_items = train, n_users, n_items

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        validate_ease_conf(conf)
        return EASE(conf['lam'])


# ---------------------------------------------------------------------------------------------------------- SLIM
def validate_slim_conf(conf: dict):
    """The SLIM keys of a conf (linear_algs.py:128): `alpha` (finite and > 0), `l1_ratio` (a number in [0, 1]) and
    `max_iter` (an integer >= 1), all required; anything else raises ValueError."""
    checks.require(conf, 'SLIM', 'alpha', 'l1_ratio', 'max_iter')
    checks.positive('alpha', conf['alpha'])
    if not 0 <= checks.number('l1_ratio', conf['l1_ratio']) <= 1:       # false for nan
        raise ValueError(f"l1_ratio = {conf['l1_ratio']!r} must be in [0, 1]")
    checks.integer('max_iter', conf['max_iter'], 1)


class SLIM(ItemWeightAlgorithm):
    """SLIM on the HIP device (algorithms/linear_algs.py:14-128 of the reference; Ning & Karypis, ICDM 2011).

    fit(X): the exact G = X^T X as EASE builds it (int8 matrix cores, nothing added to the diagonal), then
    hsk_slim_cd_f64 solves, per item j, the reference's ElasticNet(positive=True, fit_intercept=False, tol=1e-4) on X
    with column j zeroed by cyclic coordinate descent on G alone (the reference draws coordinates at random: the
    problem and the stop test are its, the iterates are the deterministic law of DESIGN.md section 5.10).  The model
    keeps the dense fp64 item x item W (W[i, j] the weight of item i for target j) and the train CSR; score_rows() is
    EASE's gather-sum, and the reference's dense users x items `pred_mtx = X @ W` is never built."""
    ALG, WEIGHTS = 'slim', 'W'
    TOL = 1e-4                 # the reference's ElasticNet(tol=...); an instance attribute `tol` overrides it
    validate_conf = staticmethod(validate_slim_conf)

    def __init__(self, alpha, l1_ratio, max_iter, device='cuda'):
        super().__init__(device)
        validate_slim_conf({'alpha': alpha, 'l1_ratio': l1_ratio, 'max_iter': max_iter})
        self.alpha, self.l1_ratio, self.max_iter = float(alpha), float(l1_ratio), int(max_iter)
        self.tol = self.TOL
        self.name = 'SLIM'
        logging.info('Built %s: alpha %s, l1_ratio %s, max_iter %d', self.name, alpha, l1_ratio, self.max_iter)

    def _forget(self):
        super()._forget()
        self.n_iter_ = self.gap_ = None

    def hyper(self) -> dict:
        return dict(alpha=np.float64(self.alpha), l1_ratio=np.float64(self.l1_ratio), max_iter=np.int64(self.max_iter))

    # ------------------------------------------------------------------ fit
    def penalties(self, n_users: int):
        """(l1, l2) of the solver: sklearn's objective times n_users."""
        return n_users * self.alpha * self.l1_ratio, n_users * self.alpha * (1 - self.l1_ratio)

    def fit_bytes(self, n_users: int, n_items: int) -> int:
        """Device bytes fit() allocates: G, Wt and W, the int8 operand of X^T, one count block and the workspace."""
        rows_pad, k_pad = hip_ops.knn_pack_dims(n_items, n_users)
        return (3 * 8 * n_items * n_items + rows_pad * k_pad + 4 * self._gram_block(n_items) * n_items +
                hip_ops.slim_ws_bytes(n_items) + 12 * n_items)

    def _solve(self, G, n_users: int):
        """(Wt, n_iter, gap) of hsk_slim_cd_f64 on the Gram G."""
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        l1, l2 = self.penalties(n_users)
        solved = hip_ops.slim_cd(G, l1, l2, self.tol, self.max_iter, status=status)
        if int(status.item()) & hip_ops.STATUS_NOT_FINITE:
            raise ValueError(f'{self.name}.fit: the solver met a non-finite value (HSK_STATUS_NOT_FINITE)')
        return solved

    def fit(self, matrix):
        indptr, indices, n_users, n_items = csr_arrays(matrix)
        self._require_free(self.fit_bytes(n_users, n_items), f'{n_items} items')
        self._forget()                    # a fit that raises leaves no model behind
        G, train = self._gram(indptr, indices, n_users, n_items, 0)
        Wt, n_iter, gap = self._solve(G, n_users)
        del G
        self.W = Wt.t().contiguous()
        self.n_iter_, self.gap_ = n_iter, gap
        self.train, self.n_users, self.n_items = train, n_users, n_items

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        validate_slim_conf(conf)
        return SLIM(conf['alpha'], conf['l1_ratio'], conf['max_iter'])
