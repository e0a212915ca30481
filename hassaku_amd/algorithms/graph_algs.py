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
import math
import os

import numpy as np
import torch

from hassaku_amd import hip_ops
from hassaku_amd.algorithms.base_classes import FittedRecommenderAlgorithm, csr_arrays


def _alpha(alpha) -> float:
    """alpha as a float, refusing what has no such value or is not positive (the reference asserts alpha >= 0, but its
    `.power(0)` raises inside scipy)."""
    if isinstance(alpha, (bool, np.bool_)) or not isinstance(alpha, (int, float, np.integer, np.floating)):
        raise ValueError(f'alpha = {alpha!r} must be a number')
    if not math.isfinite(alpha) or not alpha > 0:
        raise ValueError(f'alpha = {alpha!r} must be a finite number > 0')
    return float(alpha)


def validate_p3alpha_conf(conf: dict):
    """The P3alpha key of a conf (graph_algs.py:86-88): `alpha`, required as the reference's build_from_conf does."""
    if 'alpha' not in conf:
        raise ValueError('P3alpha conf needs alpha')
    _alpha(conf['alpha'])


class P3alpha(FittedRecommenderAlgorithm):
    GRAM_BLOCK_ROWS = 4096       # rows of W per launch of the Gram kernel (a multiple of 128)
    WINDOW = 1024                # item window of one scoring workgroup

    def __init__(self, alpha=1.9, device='cuda'):
        super().__init__(device)
        self.alpha = _alpha(alpha)
        self.name = 'P3alpha'
        self.W = None              # fp64 [n_items, n_items] on the device
        self.inv_deg_u = None      # fp64 [n_users]: 1 / user degree, 0 for users without items
        logging.info('Built %s: alpha %s', self.name, self.alpha)

    # ------------------------------------------------------------------ fit
    def fit_bytes(self, n_users: int, n_items: int) -> int:
        """Device bytes fit() allocates: W, the int8 operand of X^T and the two reciprocal-degree vectors."""
        rows_pad, k_pad = hip_ops.knn_pack_dims(n_items, n_users)
        return 8 * n_items * n_items + rows_pad * k_pad + 8 * (k_pad + n_items)

    def fit(self, matrix):
        indptr, indices, n_users, n_items = csr_arrays(matrix)
        dev = self.device
        self._require_free(self.fit_bytes(n_users, n_items), f'{n_items} items')
        self.W = self.pred_mtx = self.inv_deg_u = None     # a fit that raises leaves no model behind
        x_ptr, x_idx, t_ptr, t_idx = self._upload(indptr, indices, transpose=(n_users, n_items))
        M = hip_ops.knn_pack_i8(t_ptr, t_idx, n_items, n_users)
        w_u = hip_ops.p3_inv_degrees(x_ptr, M.shape[1])     # zero on the padding of k
        w_i = hip_ops.p3_inv_degrees(t_ptr)
        W = torch.empty((n_items, n_items), dtype=torch.float64, device=dev)
        for r0 in range(0, n_items, self.GRAM_BLOCK_ROWS):
            hip_ops.p3_gram_f64(M, n_items, w_u, r0, min(r0 + self.GRAM_BLOCK_ROWS, n_items), W, row_scale=w_i)
        del M
        self.W, self.inv_deg_u = W, w_u[:n_users].contiguous()
        self.train, self.n_users, self.n_items = (x_ptr, x_idx), n_users, n_items

    def weights(self) -> np.ndarray:
        """W as a numpy array [n_items, n_items]."""
        return self.W.cpu().numpy()

    # ------------------------------------------------------------------ scoring
    def score_rows(self, u_idxs: torch.Tensor, excl=None, out=None) -> torch.Tensor:
        u = u_idxs.to(self.device, torch.int64).contiguous()
        if self.pred_mtx is not None:
            return self._dense_rows(u, excl)
        if self.W is None:
            raise RuntimeError(f'{self.name}: run fit() or load_model_from_path() first')
        return hip_ops.p3_score_rows(u, (*self.train, self.n_users), self.W, self.inv_deg_u, self.alpha,
                                     window=self.WINDOW, excl=excl, out=out, status=self._status_word())

    # ------------------------------------------------------------------ persistence
    def save_model_to_path(self, path: str):
        np.savez(os.path.join(path, 'model.npz'), alg=np.array('p3alpha'), alpha=np.float64(self.alpha),
                 n_users=np.int64(self.n_users), n_items=np.int64(self.n_items), W=self.weights(),
                 train_indptr=self.train[0].cpu().numpy(), train_indices=self.train[1].cpu().numpy())
        logging.info('Model Saved')

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

    def load_model_from_path(self, path: str):
        dev = self.device
        with np.load(os.path.join(path, 'model.npz')) as f:       # never with allow_pickle
            if 'pred_mtx' in f:
                self._load_pred_mtx(f)
                self.W = self.inv_deg_u = None
            else:
                self._check_alg(f, 'p3alpha')
                n_users, n_items = int(f['n_users']), int(f['n_items'])
                alpha = _alpha(float(f['alpha']))
                W = f['W']
                if W.shape != (n_items, n_items):
                    raise ValueError(f'W of model.npz has shape {W.shape}, expected ({n_items}, {n_items})')
                t_ptr, t_idx = self._read_train(f, n_users, n_items)
                deg = np.diff(t_ptr)
                w_u = np.zeros(n_users, np.float64)
                w_u[deg > 0] = 1.0 / deg[deg > 0]        # one IEEE division each, as hsk_p3_inv_degrees
                self.n_users, self.n_items, self.alpha = n_users, n_items, alpha
                self.W = torch.from_numpy(np.ascontiguousarray(W, np.float64)).to(dev)
                self.inv_deg_u = torch.from_numpy(w_u).to(dev)
                self.train = self._upload(t_ptr, t_idx)
                self.pred_mtx = None
        logging.info('Model Loaded')

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        validate_p3alpha_conf(conf)
        return P3alpha(alpha=conf['alpha'])
