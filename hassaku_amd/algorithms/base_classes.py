"""Plugin base classes with the reference's method names (algorithms/base_classes.py:12-165).

Two families: `SGDBasedRecommenderAlgorithm` (trained by `Trainer`) and `SparseMatrixBasedRecommenderAlgorithm`
(fitted once on the binary train matrix: ItemKNN / UserKNN, EASE, P3alpha and SVD, which share
`FittedRecommenderAlgorithm`).  Where the reference keeps a dense float64 `pred_mtx` on the host, a sparse-matrix model
here scores chunks of user rows on the device (`score_rows`); `predict` gathers from those rows and returns float64
like the reference's.
"""
import abc
import logging
import os
from typing import Dict

import numpy as np
import torch
from torch import nn

from hassaku_amd.data.csr import UserItemCsr


class RecommenderAlgorithm(abc.ABC):
    """predict(u_idxs [B], i_idxs [B, n]) -> scores [B, n]; save/load; build_from_conf(conf, dataset)."""

    def __init__(self):
        super().__init__()
        self.name = 'RecommenderAlgorithm'

    @abc.abstractmethod
    def predict(self, u_idxs: torch.Tensor, i_idxs: torch.Tensor) -> torch.Tensor:
        ...

    @abc.abstractmethod
    def save_model_to_path(self, path: str):
        ...

    @abc.abstractmethod
    def load_model_from_path(self, path: str):
        ...

    @staticmethod
    @abc.abstractmethod
    def build_from_conf(conf: dict, dataset):
        ...


class SparseMatrixBasedRecommenderAlgorithm(RecommenderAlgorithm):
    """Models fitted on the user x item sparse matrix (algorithms/base_classes.py:55-85).  Subclasses implement
    `fit(matrix)` (a scipy CSR or a `UserItemCsr`) and `score_rows(u_idxs, excl=None)` -> float64 [B, n_items] on the
    device; `excl` = (indptr, indices) of an exclusion CSR whose columns come back as -inf."""

    def __init__(self):
        super().__init__()
        self.name = 'SparseMatrixBasedRecommenderAlgorithm'

    @abc.abstractmethod
    def fit(self, matrix):
        ...

    @abc.abstractmethod
    def score_rows(self, u_idxs: torch.Tensor, excl=None) -> torch.Tensor:
        ...

    @torch.no_grad()
    def predict(self, u_idxs: torch.Tensor, i_idxs: torch.Tensor) -> torch.Tensor:
        """float64 scores [B, n] of users u_idxs [B] on items i_idxs [B, n] (pred_mtx[u_idxs[:, None], i_idxs])."""
        rows = self.score_rows(u_idxs)
        return torch.gather(rows, 1, i_idxs.to(rows.device, torch.int64))


def csr_arrays(matrix):
    """(indptr int64, indices int32, n_rows, n_cols) of a UserItemCsr or a scipy sparse matrix (stored entries = 1)."""
    if isinstance(matrix, UserItemCsr):
        return (np.ascontiguousarray(matrix.indptr, np.int64), np.ascontiguousarray(matrix.indices, np.int32),
                matrix.n_rows, matrix.n_cols)
    m = matrix.tocsr(copy=True)
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    return (m.indptr.astype(np.int64), m.indices.astype(np.int32), m.shape[0], m.shape[1])


def csr_transpose(indptr, indices, vals, n_rows, n_cols):
    """CSR of the transpose on the device, each row's entries in ascending column order."""
    rows = torch.repeat_interleave(torch.arange(n_rows, device=indptr.device), indptr[1:] - indptr[:-1])
    order = torch.argsort(indices.long() * n_rows + rows)
    t_ptr = torch.zeros(n_cols + 1, dtype=torch.int64, device=indptr.device)
    torch.cumsum(torch.bincount(indices.long(), minlength=n_cols), 0, out=t_ptr[1:])
    return t_ptr, rows[order].to(torch.int32).contiguous(), None if vals is None else vals[order].contiguous()


class FittedRecommenderAlgorithm(SparseMatrixBasedRecommenderAlgorithm):
    """What the models fitted in closed form on the device share: where they live, the train CSR they score from, the
    dense `pred_mtx` of a reference-written model.npz, the status word of their scoring kernels and the pieces of
    fit() and load_model_from_path() that do not depend on the model."""

    def __init__(self, device='cuda'):
        super().__init__()
        self.device = torch.device(device)
        self.pred_mtx = None       # dense float64 predictions of a reference-written model.npz
        self.train = None          # (indptr int64, indices int32) of X
        self.n_users = self.n_items = None
        self._status = None

    # ------------------------------------------------------------------ fit
    def _upload(self, indptr, indices, transpose=None):
        """The host CSR of X on the device: (x_ptr, x_idx), followed, if `transpose` = (n_users, n_items) is given, by
        (t_ptr, t_idx) of X^T."""
        x = (torch.from_numpy(indptr).to(self.device), torch.from_numpy(indices).to(self.device))
        return x if transpose is None else x + csr_transpose(*x, None, *transpose)[:2]

    def _require_free(self, need: int, what: str):
        free = torch.cuda.mem_get_info(self.device)[0]
        if need > free:
            raise ValueError(f'{self.name}.fit on {what} needs {need} bytes of device memory, {free} are free')

    # ------------------------------------------------------------------ scoring
    def _status_word(self) -> torch.Tensor:
        if self._status is None:
            self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        return self._status

    def check_indices(self):
        if self._status is not None and int(self._status.item()) != 0:
            self._status.zero_()
            raise IndexError(f'{self.name}: user index outside [0, {self.n_users})')

    def _dense_rows(self, u, excl):
        rows = self.pred_mtx[u]
        if excl is not None:
            ep, ei = excl
            lens = ep[u + 1] - ep[u]
            which = torch.repeat_interleave(torch.arange(len(u), device=u.device), lens)
            starts = torch.repeat_interleave(ep[u] - (torch.cumsum(lens, 0) - lens), lens)
            cols = ei[starts + torch.arange(int(lens.sum()), device=u.device)].long()
            rows[which, cols] = -torch.inf
        return rows.contiguous()

    # ------------------------------------------------------------------ persistence
    @staticmethod
    def _read_pred_mtx(f) -> np.ndarray:
        pred = f['pred_mtx']
        if pred.ndim != 2:
            raise ValueError('pred_mtx of model.npz must be a dense 2-D array')
        return pred

    def _load_pred_mtx(self, f):
        """Takes over the dense predictions of a model.npz written by the reference; the model's own state goes."""
        pred = self._read_pred_mtx(f)
        self.pred_mtx = torch.from_numpy(np.ascontiguousarray(pred, np.float64)).to(self.device)
        self.n_users, self.n_items = pred.shape
        self.train = None

    def _check_alg(self, f, alg: str):
        if str(f['alg']) != alg:
            raise ValueError(f"model.npz holds a {str(f['alg'])} model, not {self.name}")

    @staticmethod
    def _read_train(f, n_users: int, n_items: int, validate=True):
        """(indptr int64, indices int32) of the train CSR of a model.npz, on the host."""
        t_ptr, t_idx = f['train_indptr'], f['train_indices']
        if validate and (t_ptr.shape != (n_users + 1,) or t_ptr[0] != 0 or np.any(np.diff(t_ptr) < 0) or
                         t_ptr[-1] != len(t_idx) or
                         (len(t_idx) and not (0 <= t_idx.min() and t_idx.max() < n_items))):
            raise ValueError(f'train CSR of model.npz does not describe {n_users} users x {n_items} items')
        return np.ascontiguousarray(t_ptr, np.int64), np.ascontiguousarray(t_idx, np.int32)


class SGDBasedRecommenderAlgorithm(RecommenderAlgorithm, nn.Module):
    """Models trained by mini-batch SGD through `Trainer` (algorithms/base_classes.py:88-165)."""

    def __init__(self):
        super().__init__()
        self.name = 'SGDBasedRecommenderAlgorithm'

    def forward(self, u_idxs: torch.Tensor, i_idxs: torch.Tensor) -> torch.Tensor:
        return self.combine_user_item_representations(self.get_user_representations(u_idxs),
                                                      self.get_item_representations(i_idxs))

    @abc.abstractmethod
    def get_user_representations(self, u_idxs: torch.Tensor):
        ...

    @abc.abstractmethod
    def get_item_representations(self, i_idxs: torch.Tensor):
        ...

    @abc.abstractmethod
    def combine_user_item_representations(self, u_repr, i_repr) -> torch.Tensor:
        ...

    def get_and_reset_other_loss(self) -> Dict:
        """At least {'reg_loss': tensor[1]}; MF has no extra loss (algorithms/base_classes.py:139-148)."""
        return {'reg_loss': torch.zeros(1)}

    @torch.no_grad()
    def predict(self, u_idxs: torch.Tensor, i_idxs: torch.Tensor) -> torch.Tensor:
        self.eval()
        return self(u_idxs, i_idxs)

    def save_model_to_path(self, path: str):
        hook = getattr(self, '_pre_save_hook', None)   # a fused trainer registers its flush(): no lazily updated row
        if callable(hook):                             # reaches the checkpoint with pending zero-gradient steps
            hook()
        torch.save(self.state_dict(), os.path.join(path, 'model.pth'))
        logging.info('Model Saved')

    def load_model_from_path(self, path: str):
        device = next(self.parameters()).device
        self.load_state_dict(torch.load(os.path.join(path, 'model.pth'), map_location=device))
        logging.info('Model Loaded')
