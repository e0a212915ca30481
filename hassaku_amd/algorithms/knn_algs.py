"""ItemKNN / UserKNN on the HIP device (algorithms/knn_algs.py and utilities/similarities.py of the reference).

fit(X), X the binary user x item train matrix:
  * the entity matrix M (X^T for ItemKNN, X for UserKNN) is packed into a dense int8 operand (hsk_knn_pack_i8);
  * per block of rows the co-occurrence counts C = M M^T come from the int8 matrix cores (hsk_knn_gram_i8, exact
    int32), and every row's fp64 similarities and its k nearest neighbours from hsk_knn_select;
  * the neighbours are kept as a CSR S in the reference's stored order (value desc, index asc).
Predictions are never materialised as a dense users x items matrix: score_rows() computes the float64 rows of
X S^T (ItemKNN) or S X (UserKNN) for a chunk of users with hsk_knn_score_rows, adding in scipy's order, so each row is
bitwise the reference's `pred_mtx` row ("KNN").
"""
import logging
import os
from enum import Enum

import numpy as np
import torch

from hassaku_amd import hip_ops
from hassaku_amd.algorithms.base_classes import FittedRecommenderAlgorithm, csr_arrays, csr_transpose
from hassaku_amd.conf import checks


class SimilarityFunctionEnum(Enum):
    """The reference's five similarity names (utilities/similarities.py:105-110); values = HSK_KNN_* kinds."""
    cosine = 0
    jaccard = 1
    sorensen_dice = 2
    asymmetric_cosine = 3
    tversky = 4


def _needs(sim: SimilarityFunctionEnum):
    return {SimilarityFunctionEnum.asymmetric_cosine: ('alpha',),
            SimilarityFunctionEnum.tversky: ('alpha', 'beta')}.get(sim, ())


def validate_knn_conf(conf: dict):
    """The KNN keys of a conf (knn_algs.py:62-72): raises ValueError on what the reference would only trip over
    inside fit (a missing alpha / beta) or not at all (k outside [1, 1024])."""
    params = conf.get('sim_func_params')
    if not isinstance(params, dict) or 'sim_func_name' not in params:
        raise ValueError('KNN conf needs sim_func_params.sim_func_name')
    name = params['sim_func_name']
    if name not in SimilarityFunctionEnum.__members__:
        raise ValueError(f'sim_func_name {name!r} is not one of {list(SimilarityFunctionEnum.__members__)}')
    for key in _needs(SimilarityFunctionEnum[name]):
        if params.get(key) is None:
            raise ValueError(f'sim_func_name {name} needs sim_func_params.{key}')
    checks.require(conf, 'KNN', 'k')
    checks.integer('k', conf['k'], 1, hip_ops.KNN_MAX_K)
    if not checks.number('shrinkage', conf.get('shrinkage', 0.)) >= 0:
        raise ValueError(f"shrinkage = {conf['shrinkage']!r} must be a number >= 0")


_transpose = csr_transpose     # the name this module had it under; tests/test_ease.py and test_p3alpha.py import it

class KNNAlgorithm(FittedRecommenderAlgorithm):
    """Common part of UserKNN / ItemKNN (knn_algs.py:13-72)."""
    WINDOW = 4096                # item window of one scoring wave (fp64 accumulators in LDS)
    ITEM_BASED = False
    validate_conf = staticmethod(validate_knn_conf)

    def __init__(self, sim_func_enum: SimilarityFunctionEnum = SimilarityFunctionEnum.cosine, k: int = 100,
                 shrinkage: float = .0, device='cuda', **kwargs):
        super().__init__(device)
        if isinstance(sim_func_enum, str):
            sim_func_enum = SimilarityFunctionEnum[sim_func_enum]
        for key in _needs(sim_func_enum):
            if kwargs.get(key) is None:
                raise ValueError(f'{sim_func_enum.name} similarity needs {key}')
        if not 1 <= int(k) <= hip_ops.KNN_MAX_K:
            raise ValueError(f'k = {k} outside [1, {hip_ops.KNN_MAX_K}]')
        self.sim_func_enum = sim_func_enum
        self.alpha, self.beta = kwargs.get('alpha'), kwargs.get('beta')
        self.k, self.shrinkage = int(k), float(shrinkage)
        self.name = 'KNNAlgorithm'
        logging.info('Built %s: sim_func %s, k %d, shrinkage %s', self.name, sim_func_enum.name, self.k, self.shrinkage)

    def _forget(self):
        super()._forget()
        self.neigh = None          # (indptr int64, indices int32, vals fp64) of S, stored order
        self._b_t = None           # S^T (ItemKNN scoring)

    # ------------------------------------------------------------------ fit
    def _pack(self, indptr, indices, n_users, n_items):
        """Uploads X as the train CSR and packs the entity matrix (X^T for ItemKNN, X for UserKNN): (the dense int8
        operand, its number of rows, the degree vectors hsk_knn_select reads: deg, sqrt, deg^alpha, deg^(1-alpha))."""
        dev = self.device
        up = self._upload(indptr, indices, transpose=(n_users, n_items) if self.ITEM_BASED else None)
        self.train, self.n_users, self.n_items = up[:2], n_users, n_items
        (e_ptr, e_idx), (n_ent, n_feat) = up[-2:], (n_items, n_users) if self.ITEM_BASED else (n_users, n_items)
        deg = np.diff(e_ptr.cpu().numpy()).astype(np.int64)
        sim = self.sim_func_enum
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)  # noqa: E731
        sq = put(np.sqrt(deg.astype(np.float64))) if sim == SimilarityFunctionEnum.cosine else None
        pa = p1a = None
        if sim == SimilarityFunctionEnum.asymmetric_cosine:
            pa, p1a = put(np.power(deg, self.alpha)), put(np.power(deg, 1 - self.alpha))
        deg_d = torch.from_numpy(deg).to(dev)
        return hip_ops.knn_pack_i8(e_ptr, e_idx, n_ent, n_feat), n_ent, (deg_d, sq, pa, p1a)

    def _select(self, C, r0: int, r1: int, degrees):
        """(idx, val, len) of the k nearest neighbours of rows [r0, r1) from their count block."""
        return hip_ops.knn_select(C, r1 - r0, r0, *degrees, self.sim_func_enum.name, self.alpha, self.beta,
                                  self.shrinkage, min(self.k, hip_ops.KNN_MAX_K))

    def fit(self, matrix):
        dev = self.device
        M, n_ent, degrees = self._pack(*csr_arrays(matrix))
        k = min(self.k, hip_ops.KNN_MAX_K)
        idx = torch.empty((n_ent, k), dtype=torch.int32, device=dev)
        val = torch.empty((n_ent, k), dtype=torch.float64, device=dev)
        ln = torch.empty(n_ent, dtype=torch.int32, device=dev)
        for r0, r1, C in self._count_blocks(M, n_ent):
            idx[r0:r1], val[r0:r1], ln[r0:r1] = self._select(C, r0, r1, degrees)
        del M, C
        keep = torch.arange(k, device=dev)[None, :] < ln[:, None]
        s_ptr = torch.zeros(n_ent + 1, dtype=torch.int64, device=dev)
        torch.cumsum(ln.long(), 0, out=s_ptr[1:])
        self.neigh = (s_ptr, idx[keep].contiguous(), val[keep].contiguous())
        self.pred_mtx, self._b_t = None, None

    def neighbours(self):
        """(indptr, indices, data) numpy arrays of the neighbour CSR S (rows in the reference's stored order)."""
        return tuple(t.cpu().numpy() for t in self.neigh)

    # ------------------------------------------------------------------ scoring
    def _operands(self):
        s_ptr, s_idx, s_val = self.neigh
        x_ptr, x_idx = self.train
        if self.ITEM_BASED:          # pred = X S^T: the user's items in ascending order pick rows of S^T
            if self._b_t is None:
                self._b_t = csr_transpose(s_ptr, s_idx, s_val, self.n_items, self.n_items)
            return (x_ptr, x_idx, None, self.n_users), (*self._b_t, self.n_items)
        return (s_ptr, s_idx, s_val, self.n_users), (x_ptr, x_idx, None, self.n_users)   # pred = S X

    def score_rows(self, u_idxs: torch.Tensor, excl=None, out=None) -> torch.Tensor:
        u = u_idxs.to(self.device, torch.int64).contiguous()
        if self.pred_mtx is not None:
            return self._dense_rows(u, excl)
        if self.neigh is None:
            raise RuntimeError(f'{self.name}: run fit() or load_model_from_path() first')
        a, b = self._operands()
        return hip_ops.knn_score_rows(u, a, b, self.n_items, window=self.WINDOW, excl=excl, out=out,
                                      status=self._status_word())

    # ------------------------------------------------------------------ persistence
    def save_model_to_path(self, path: str):
        s_ptr, s_idx, s_val = self.neighbours()
        np.savez(os.path.join(path, 'model.npz'), alg=np.array('iknn' if self.ITEM_BASED else 'uknn'),
                 k=np.int64(self.k), n_users=np.int64(self.n_users), n_items=np.int64(self.n_items),
                 neigh_indptr=s_ptr, neigh_indices=s_idx, neigh_data=s_val,
                 train_indptr=self.train[0].cpu().numpy(), train_indices=self.train[1].cpu().numpy())
        logging.info('Model Saved')

    def load_model_from_path(self, path: str):
        dev = self.device
        self._forget()                # a load that raises leaves no model behind
        with np.load(os.path.join(path, 'model.npz')) as f:
            if 'pred_mtx' in f:       # written by the reference (knn_algs.py:46-56): dense float64 predictions
                self._load_pred_mtx(f)
            else:
                self._check_alg(f, 'iknn' if self.ITEM_BASED else 'uknn')
                self.n_users, self.n_items = int(f['n_users']), int(f['n_items'])
                self.neigh = (torch.from_numpy(f['neigh_indptr']).to(dev), torch.from_numpy(f['neigh_indices']).to(dev),
                              torch.from_numpy(f['neigh_data']).to(dev))
                self.train = self._upload(*self._read_train(f, self.n_users, self.n_items, validate=False))
        logging.info('Model Loaded')

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        validate_knn_conf(conf)
        params = conf['sim_func_params']
        cls = UserKNN if conf.get('alg') == 'uknn' else ItemKNN
        return cls(SimilarityFunctionEnum[params['sim_func_name']], conf['k'], conf.get('shrinkage', .0),
                   alpha=params.get('alpha'), beta=params.get('beta'))


class UserKNN(KNNAlgorithm):
    """Neighbours among users; pred = S X (knn_algs.py:104-121)."""
    ITEM_BASED = False

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.name = 'UserKNN'


class ItemKNN(KNNAlgorithm):
    """Neighbours among items; pred = X S^T (knn_algs.py:124-140)."""
    ITEM_BASED = True

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.name = 'ItemKNN'
