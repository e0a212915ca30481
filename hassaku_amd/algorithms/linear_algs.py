"""EASE on the HIP device (algorithms/linear_algs.py:131-176 of the reference; Steck, arXiv:1905.03375).

fit(X), X the binary user x item train matrix:
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
from hassaku_amd.algorithms.base_classes import SparseMatrixBasedRecommenderAlgorithm
from hassaku_amd.algorithms.knn_algs import KNNAlgorithm, _csr_arrays, _transpose


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


class EASE(SparseMatrixBasedRecommenderAlgorithm):
    GRAM_BLOCK_BYTES = 1 << 30   # int32 counts of one row block
    WINDOW = 1024                # item window of one scoring workgroup

    def __init__(self, lam, device='cuda'):
        super().__init__()
        self.lam = lam
        self.lam_int = _lam_int(lam)
        self.device = torch.device(device)
        self.name = 'EASE'
        self.pred_mtx = None       # dense float64 predictions of a reference-written model.npz
        self.B = None              # fp64 [n_items, n_items] on the device
        self.train = None          # (indptr int64, indices int32) of X
        self.n_users = self.n_items = None
        self._status = None
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
        indptr, indices, n_users, n_items = _csr_arrays(matrix)
        dev = self.device
        need = self.fit_bytes(n_users, n_items)
        free = torch.cuda.mem_get_info(dev)[0]
        if need > free:
            raise ValueError(f'EASE.fit on {n_items} items needs {need} bytes of device memory, {free} are free')
        self.B = self.pred_mtx = None     # a fit that raises leaves no model behind, not the old B on a new matrix
        x_ptr, x_idx = torch.from_numpy(indptr).to(dev), torch.from_numpy(indices).to(dev)
        t_ptr, t_idx, _ = _transpose(x_ptr, x_idx, None, n_users, n_items)
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
    _dense_rows = KNNAlgorithm._dense_rows

    def score_rows(self, u_idxs: torch.Tensor, excl=None, out=None) -> torch.Tensor:
        u = u_idxs.to(self.device, torch.int64).contiguous()
        if self.pred_mtx is not None:
            return self._dense_rows(u, excl)
        if self.B is None:
            raise RuntimeError(f'{self.name}: run fit() or load_model_from_path() first')
        if self._status is None:
            self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        return hip_ops.ease_score_rows(u, (*self.train, self.n_users), self.B, window=self.WINDOW, excl=excl, out=out,
                                       status=self._status)

    def check_indices(self):
        if self._status is not None and int(self._status.item()) != 0:
            self._status.zero_()
            raise IndexError(f'{self.name}: user index outside [0, {self.n_users})')

    # ------------------------------------------------------------------ persistence
    def save_model_to_path(self, path: str):
        np.savez(os.path.join(path, 'model.npz'), alg=np.array('ease'), lam=np.float64(self.lam),
                 n_users=np.int64(self.n_users), n_items=np.int64(self.n_items), B=self.weights(),
                 train_indptr=self.train[0].cpu().numpy(), train_indices=self.train[1].cpu().numpy())
        logging.info('Model Saved')

    def load_model_from_path(self, path: str):
        dev = self.device
        with np.load(os.path.join(path, 'model.npz')) as f:
            if 'pred_mtx' in f:       # written by the reference (linear_algs.py:163-166): dense float64 predictions
                pred = f['pred_mtx']
                if pred.ndim != 2:
                    raise ValueError('pred_mtx of model.npz must be a dense 2-D array')
                self.pred_mtx = torch.from_numpy(np.ascontiguousarray(pred, np.float64)).to(dev)
                self.n_users, self.n_items = pred.shape
                self.B = self.train = None
            else:
                alg = str(f['alg'])
                if alg != 'ease':
                    raise ValueError(f'model.npz holds a {alg} model, not {self.name}')
                n_users, n_items = int(f['n_users']), int(f['n_items'])
                B, t_ptr, t_idx = f['B'], f['train_indptr'], f['train_indices']
                if B.shape != (n_items, n_items):
                    raise ValueError(f'B of model.npz has shape {B.shape}, expected ({n_items}, {n_items})')
                if (t_ptr.shape != (n_users + 1,) or t_ptr[0] != 0 or np.any(np.diff(t_ptr) < 0) or
                        t_ptr[-1] != len(t_idx) or (len(t_idx) and not (0 <= t_idx.min() and t_idx.max() < n_items))):
                    raise ValueError(f'train CSR of model.npz does not describe {n_users} users x {n_items} items')
                self.n_users, self.n_items = n_users, n_items
                self.B = torch.from_numpy(np.ascontiguousarray(B, np.float64)).to(dev)
                self.train = (torch.from_numpy(np.ascontiguousarray(t_ptr, np.int64)).to(dev),
                              torch.from_numpy(np.ascontiguousarray(t_idx, np.int32)).to(dev))
                self.pred_mtx = None
        logging.info('Model Loaded')

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        validate_ease_conf(conf)
        return EASE(conf['lam'])
