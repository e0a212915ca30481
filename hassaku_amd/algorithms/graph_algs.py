"""P3alpha on the HIP device (algorithms/graph_algs.py:9-88 of the reference; Cooper et al., WWW 2014 companion).

The reference builds the (users + items)^2 transition matrix P = D^-1 A, takes P ** 3, keeps the user x item block and
raises it element-wise to alpha.  Restricted to that block, with X the binary user x item train matrix, d the degrees
and w = 1 / d (0 where d = 0):
    S = X^T diag(w_u) X,   W = diag(w_i) S,   pred[u, j] = (w_u * sum_{i in items(u)} W[i, j]) ^ alpha.
fit(X):
  * hsk_p3_inv_degrees gives w_u (padded to the int8 operand's k) and w_i;
  * X^T is packed into the dense int8 operand of the neighbourhood models (hsk_knn_pack_i8);
  * hsk_p3_gram_f64 computes W block by block on the fp64 matrix cores, converting the int8 image on the fly.
The item x item W is what the model keeps.  Neither the reference's users x items `pred_mtx` nor its (users + items)^2
intermediates are built: score_rows() sums, per user, the rows of W its items pick, in ascending item order from 0.0,
scales by w_u and raises to alpha.  Every term is positive, so the distance to the reference is
bounded by the number of three-step paths, whatever order either side adds in.
"""
import logging

import numpy as np
import torch

from hassaku_amd import hip_ops
from hassaku_amd.algorithms.base_classes import ItemWeightAlgorithm, csr_arrays
from hassaku_amd.conf import checks


def validate_p3alpha_conf(conf: dict):
    """The P3alpha key of a conf (graph_algs.py:86-88): `alpha`, required as the reference's build_from_conf does;
    finite and > 0 (the reference asserts alpha >= 0, but its `.power(0)` raises inside scipy)."""
    checks.require(conf, 'P3alpha', 'alpha')
    checks.positive('alpha', conf['alpha'])


class P3alpha(ItemWeightAlgorithm):
    ALG, WEIGHTS = 'p3alpha', 'W'
    GRAM_BLOCK_ROWS = 4096       # rows of W per launch of the Gram kernel (a multiple of 128)
    validate_conf = staticmethod(validate_p3alpha_conf)

    def __init__(self, alpha=1.9, device='cuda'):
        super().__init__(device)
        self.alpha = checks.positive('alpha', alpha)
        self.name = 'P3alpha'
        logging.info('Built %s: alpha %s', self.name, self.alpha)

    def _forget(self):
        super()._forget()
        self.inv_deg_u = None      # fp64 [n_users]: 1 / user degree, 0 for users without items

    def hyper(self) -> dict:
        return dict(alpha=np.float64(self.alpha))

    # ------------------------------------------------------------------ fit
    def fit_bytes(self, n_users: int, n_items: int) -> int:
        """Device bytes fit() allocates: W, the int8 operand of X^T and the two reciprocal-degree vectors."""
        rows_pad, k_pad = hip_ops.knn_pack_dims(n_items, n_users)
        return 8 * n_items * n_items + rows_pad * k_pad + 8 * (k_pad + n_items)

    @staticmethod
    def _degrees(x_ptr, t_ptr, k_pad: int):
        """(w_u padded with zeros to the operand's k, w_i)."""
        return hip_ops.p3_inv_degrees(x_ptr, k_pad), hip_ops.p3_inv_degrees(t_ptr)

    def _weighted_gram(self, M, n_items: int, w_u, w_i):
        W = torch.empty((n_items, n_items), dtype=torch.float64, device=self.device)
        for r0 in range(0, n_items, self.GRAM_BLOCK_ROWS):
            hip_ops.p3_gram_f64(M, n_items, w_u, r0, min(r0 + self.GRAM_BLOCK_ROWS, n_items), W, row_scale=w_i)
        return W

    def fit(self, matrix):
        indptr, indices, n_users, n_items = csr_arrays(matrix)
        self._require_free(self.fit_bytes(n_users, n_items), f'{n_items} items')
        self._forget()                    # a fit that raises leaves no model behind
        train, t_ptr, M = self._pack(indptr, indices, n_users, n_items)
        w_u, w_i = self._degrees(train[0], t_ptr, M.shape[1])
        self.W = self._weighted_gram(M, n_items, w_u, w_i)
        self.inv_deg_u = w_u[:n_users].contiguous()
        self.train, self.n_users, self.n_items = train, n_users, n_items

    # ------------------------------------------------------------------ scoring
    def _score(self, u, W, **kw):
        return hip_ops.p3_score_rows(u, (*self.train, self.n_users), W, self.inv_deg_u, self.alpha, **kw)

    # ------------------------------------------------------------------ persistence
    @staticmethod
    def _read_pred_mtx(f) -> np.ndarray:
        try:
            pred = f['pred_mtx']
        except ValueError as e:
            # graph_algs.py:74-77 hands np.savez its scipy sparse pred_mtx, which numpy pickles as an object
            # array; the reference's own np.load (graph_algs.py:79-83) cannot read that back either
            raise ValueError('pred_mtx of model.npz is an object array (the pickled sparse matrix the '
                             "reference's P3alpha writes and cannot read back itself); it is not loaded: "
                             'save the dense rows (pred_mtx.toarray()) instead') from e
        if pred.dtype == object:
            raise ValueError('pred_mtx of model.npz is an object array (the pickled sparse matrix the '
                             "reference's P3alpha writes and cannot read back itself); it is not loaded")
        if pred.ndim != 2 or not np.issubdtype(pred.dtype, np.floating):
            raise ValueError('pred_mtx of model.npz must be a dense 2-D float array')
        return pred

    def _load_own(self, f, t_ptr):
        self.alpha = checks.positive('alpha', float(f['alpha']))
        deg = np.diff(t_ptr)
        w_u = np.zeros(len(deg), np.float64)
        w_u[deg > 0] = 1.0 / deg[deg > 0]        # one IEEE division each, as hsk_p3_inv_degrees
        self.inv_deg_u = torch.from_numpy(w_u).to(self.device)

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        validate_p3alpha_conf(conf)
        return P3alpha(alpha=conf['alpha'])
