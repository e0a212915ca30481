"""Plugin base classes with the reference's method names (algorithms/base_classes.py:12-165).

Two families: `SGDBasedRecommenderAlgorithm` (trained by `Trainer`) and `SparseMatrixBasedRecommenderAlgorithm`
(fitted once on the binary train matrix).  The seven fitted models share `FittedRecommenderAlgorithm`: ItemKNN /
UserKNN keep a neighbour CSR of their own; EASE, SLIM and P3alpha are `ItemWeightAlgorithm`s (a dense fp64 item x item
matrix, the train CSR and the gather-sum scorer); SVD and ALS are `FactorAlgorithm`s (two padded fp64 factor blocks).
Where the reference keeps a dense float64 `pred_mtx` on the host, a sparse-matrix model here scores chunks of user rows
on the device (`score_rows`); `predict` gathers from those rows and returns float64 like the reference's.
"""
import abc
import logging
import os
from typing import Dict

import numpy as np
import torch
from torch import nn

from hassaku_amd import hip_ops
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

    @staticmethod
    def validate_conf(conf: dict):
        """Raises ValueError on the model's own conf keys; parse_conf calls it.  A model without such keys checks
        nothing."""


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
    GRAM_BLOCK_BYTES = 1 << 30   # int32 counts of one row block of _count_blocks(); an instance may override it

    def __init__(self, device='cuda'):
        super().__init__()
        self.device = torch.device(device)
        self._status = None
        self._forget()

    def _forget(self):
        """No model: what a fit or a load starts from, so that one that raises leaves nothing behind."""
        self.pred_mtx = None       # dense float64 predictions of a reference-written model.npz
        self.train = None          # (indptr int64, indices int32) of X
        self.n_users = self.n_items = None

    # ------------------------------------------------------------------ fit
    def _upload(self, indptr, indices, transpose=None):
        """The host CSR of X on the device: (x_ptr, x_idx), followed, if `transpose` = (n_users, n_items) is given, by
        (t_ptr, t_idx) of X^T."""
        x = (torch.from_numpy(indptr).to(self.device), torch.from_numpy(indices).to(self.device))
        return x if transpose is None else x + csr_transpose(*x, None, *transpose)[:2]

    def _gram_block(self, n: int) -> int:
        """Rows of one count block of an n-row operand: a multiple of 128 within GRAM_BLOCK_BYTES, at least 128."""
        block = max(128, (self.GRAM_BLOCK_BYTES // (4 * n)) // 128 * 128)
        return min(block, -(-n // 128) * 128)

    def _count_blocks(self, M, n: int):
        """Yields (r0, r1, C): the exact int32 counts C[r - r0, c] = <M[r], M[c]> of rows [r0, r1) of the packed int8
        operand M (hsk_knn_gram_i8), block after block into one buffer."""
        block = self._gram_block(n)
        C = torch.empty((block, n), dtype=torch.int32, device=self.device)
        for r0 in range(0, n, block):
            r1 = min(r0 + block, n)
            hip_ops.knn_gram_i8(M, n, r0, r1, out=C)
            yield r0, r1, C

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
        """Takes over the dense predictions of a model.npz written by the reference (after _forget())."""
        pred = self._read_pred_mtx(f)
        self.pred_mtx = torch.from_numpy(np.ascontiguousarray(pred, np.float64)).to(self.device)
        self.n_users, self.n_items = pred.shape

    def _check_alg(self, f, alg: str):
        if 'alg' not in f:
            raise ValueError(f'model.npz has no alg key: it is not a {self.name} model written here')
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


class ItemWeightAlgorithm(FittedRecommenderAlgorithm):
    """A dense fp64 item x item matrix, the train CSR and the gather-sum scorer: EASE, SLIM and P3alpha.  A subclass
    names ALG (its registry tag), WEIGHTS (its matrix: the public attribute and the model.npz key) and hyper() (its
    hyper-parameters as saved); P3alpha also overrides _score() and _load_own()."""
    ALG = WEIGHTS = None
    WINDOW = 1024                # item window of one scoring workgroup

    def _forget(self):
        super()._forget()
        setattr(self, self.WEIGHTS, None)     # fp64 [n_items, n_items] on the device

    @abc.abstractmethod
    def hyper(self) -> dict:
        ...

    # ------------------------------------------------------------------ fit
    def _pack(self, indptr, indices, n_users, n_items):
        """((x_ptr, x_idx) of X, t_ptr of X^T, the dense int8 operand of X^T) on the device."""
        x_ptr, x_idx, t_ptr, t_idx = self._upload(indptr, indices, transpose=(n_users, n_items))
        return (x_ptr, x_idx), t_ptr, hip_ops.knn_pack_i8(t_ptr, t_idx, n_items, n_users)

    def _gram_f64(self, M, n_items, lam: int):
        """The exact fp64 G = X^T X + lam I from the count blocks of M."""
        G = torch.empty((n_items, n_items), dtype=torch.float64, device=self.device)
        for r0, r1, C in self._count_blocks(M, n_items):
            hip_ops.ease_gram_f64(C, r1 - r0, r0, lam, G)
        return G

    def _gram(self, indptr, indices, n_users, n_items, lam: int):
        """(G, the uploaded train CSR); the operand and the count block are gone when it returns."""
        train, _, M = self._pack(indptr, indices, n_users, n_items)
        return self._gram_f64(M, n_items, lam), train

    def weights(self) -> np.ndarray:
        """The item x item matrix as a numpy array [n_items, n_items]."""
        return getattr(self, self.WEIGHTS).cpu().numpy()

    # ------------------------------------------------------------------ scoring
    def _score(self, u, W, **kw):
        return hip_ops.ease_score_rows(u, (*self.train, self.n_users), W, **kw)

    def score_rows(self, u_idxs: torch.Tensor, excl=None, out=None) -> torch.Tensor:
        W = getattr(self, self.WEIGHTS)
        if self.pred_mtx is None and W is None:
            raise RuntimeError(f'{self.name}: run fit() or load_model_from_path() first')
        u = u_idxs.to(self.device, torch.int64).contiguous()
        if self.pred_mtx is not None:
            return self._dense_rows(u, excl)
        return self._score(u, W, window=self.WINDOW, excl=excl, out=out, status=self._status_word())

    # ------------------------------------------------------------------ persistence
    def save_model_to_path(self, path: str):
        np.savez(os.path.join(path, 'model.npz'), alg=np.array(self.ALG), **self.hyper(),
                 n_users=np.int64(self.n_users), n_items=np.int64(self.n_items), **{self.WEIGHTS: self.weights()},
                 train_indptr=self.train[0].cpu().numpy(), train_indices=self.train[1].cpu().numpy())
        logging.info('Model Saved')

    def _load_own(self, f, t_ptr):
        """What a subclass reads from an open model.npz beyond the matrix and the train CSR (validated first)."""

    def load_model_from_path(self, path: str):
        self._forget()                # a load that raises leaves no model behind
        with np.load(os.path.join(path, 'model.npz')) as f:       # never with allow_pickle
            if 'pred_mtx' in f:       # written by the reference: dense float64 predictions
                self._load_pred_mtx(f)
            else:
                self._check_alg(f, self.ALG)
                n_users, n_items = int(f['n_users']), int(f['n_items'])
                W = f[self.WEIGHTS]
                if W.shape != (n_items, n_items) or W.dtype.kind != 'f':
                    raise ValueError(f'{self.WEIGHTS} of model.npz is {W.dtype} {W.shape}, expected floats '
                                     f'({n_items}, {n_items})')
                train = self._read_train(f, n_users, n_items)
                self._load_own(f, train[0])
                self.n_users, self.n_items = n_users, n_items
                setattr(self, self.WEIGHTS, torch.from_numpy(np.ascontiguousarray(W, np.float64)).to(self.device))
                self.train = self._upload(*train)
        logging.info('Model Loaded')


class FactorAlgorithm(FittedRecommenderAlgorithm):
    """Two fp64 factor blocks scored on the matrix cores, and the reference's two-key model.npz: SVD and ALS.  A
    subclass names ALG (its registry tag), WIDTH (its number of factors: the attribute and the model.npz key), MAX_K
    and hyper() (what it saves beyond the factors and `alg`); SVD also overrides _load_own().  pred_mtx and train stay
    None: the factors are all a model or a file holds."""
    ALG = WIDTH = MAX_K = None

    def _forget(self):
        super()._forget()
        self.users_factors = None     # fp64 [n_users, k] on the device; a view of an even-stride buffer
        self.items_factors = None     # fp64 [n_items, k]

    @abc.abstractmethod
    def hyper(self) -> dict:
        ...

    def _padded(self, a: np.ndarray) -> torch.Tensor:
        """[n, k] float64 on the device as a view of an even-stride buffer (16-byte aligned rows for any k)."""
        buf = np.zeros((a.shape[0], hip_ops.svd_ld(a.shape[1])), np.float64)
        buf[:, :a.shape[1]] = a
        return torch.from_numpy(buf).to(self.device)[:, :a.shape[1]]

    def score_rows(self, u_idxs: torch.Tensor, excl=None, out=None) -> torch.Tensor:
        if self.items_factors is None:
            raise RuntimeError(f'{self.name}: run fit() or load_model_from_path() first')
        u = u_idxs.to(self.device, torch.int64).contiguous()
        return hip_ops.svd_score_rows(u, self.users_factors, self.items_factors, excl=excl, out=out,
                                      status=self._status_word())

    # ------------------------------------------------------------------ persistence
    def save_model_to_path(self, path: str):
        """The reference's two keys plus alg and hyper(), which its loader ignores."""
        np.savez(os.path.join(path, 'model.npz'), users_factors=self.users_factors.cpu().numpy(),
                 items_factors=self.items_factors.cpu().numpy(), alg=np.array(self.ALG), **self.hyper())
        logging.info('Model Saved')

    def _read_factors(self, f):
        """(users_factors, items_factors, k) of an open model.npz written here (`alg` must match) or by the reference
        (no `alg` key; any float dtype), validated: two 2-D float arrays that share a number of factors in [1, MAX_K]
        which the file's WIDTH key, if it has one, states too."""
        if 'alg' in f:
            self._check_alg(f, self.ALG)
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
        if vf.shape[1] != k or not 1 <= k <= self.MAX_K or uf.shape[0] < 1 or vf.shape[0] < 1:
            raise ValueError(f'users_factors {uf.shape} and items_factors {vf.shape} of model.npz do not share a '
                             f'number of factors in [1, {self.MAX_K}]')
        if self.WIDTH in f and int(f[self.WIDTH]) != k:
            raise ValueError(f'{self.WIDTH} = {int(f[self.WIDTH])} of model.npz, but the factors have {k} columns')
        return uf, vf, k

    def _load_own(self, f, k: int):
        """What a subclass reads from an open model.npz beyond the factors (validated first)."""

    def load_model_from_path(self, path: str):
        """Reads a file written here or by the reference (no `alg` key; float32 from `implicit`, or from svds on the
        float32 cast of an integer matrix -- any float dtype is taken and held as float64)."""
        self._forget()                # a load that raises leaves no model behind
        with np.load(os.path.join(path, 'model.npz')) as f:       # never with allow_pickle
            uf, vf, k = self._read_factors(f)
            self._load_own(f, k)
        setattr(self, self.WIDTH, k)
        self.n_users, self.n_items = uf.shape[0], vf.shape[0]
        self.users_factors, self.items_factors = self._padded(uf), self._padded(vf)
        logging.info('Model Loaded')


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
