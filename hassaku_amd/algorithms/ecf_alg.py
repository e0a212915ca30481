"""ECF, Explainable Collaborative Filtering with taste clusters -- algorithms/sgd_alg.py:579-775 of the reference (Du et
al., "Towards Explainable Collaborative Filtering with Taste Clusters Learning", WWW 2023).

Items are affiliated to `top_m` of `n_clusters` taste clusters by the cosine of their embedding to the cluster
embeddings, users to `top_n` clusters by the summed similarities of their train items; the score is the dot product of
the two sparse affiliation vectors.  Three extra losses shape the clusters: tag similarity (a cluster should be
describable by few tags), independence (clusters should differ) and an in-model BPR term on the plain embeddings.

The reference holds the train matrix as a dense [n_users, n_items] fp32 tensor and the weighted tag matrix as a dense
[n_items, n_tags] one and multiplies by both in every step.  Here the model holds the CSR of X, the CSR of the
transposed 0/1 tag incidence and the per-tag weights; both products are the gather-sum `hip_ops.sparse_rows_sum`
(stored entries count as 1), and the affiliation -- exact top-k mask, softmax as its straight-through estimator, sigmoid
-- is one HIP kernel each way, `hip_ops.ecf_affiliation`.  The cosine GEMM [n_items, D] x [D, n_clusters], the
log-softmaxes and the top-p over tags are dense algebra on [*, <= 64] blocks and run on the library path.

Same constructor arguments and defaults, RNG consumption at construction, state_dict() keys (`user_embed.weight`,
`item_embed.weight`, `clusters`) and `get_and_reset_other_loss()` keys as the reference's class.  Where a row of
similarities holds equal values across the top-k boundary the lower cluster index wins (torch.topk leaves it open).
"""
import inspect
import logging
import os
from typing import Dict, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from hassaku_amd import hip_ops
from hassaku_amd.algorithms.base_classes import csr_arrays
from hassaku_amd.algorithms.proto_alg import _HipTables, _pairwise_dot, cosine_to

INT_KEYS = ('embedding_dim', 'n_clusters', 'top_n', 'top_m', 'top_p')
TEMP_KEYS = ('temp_masking', 'temp_tags')


def ecf_defaults() -> dict:
    """The constructor's defaults, by name (what the reference's build_from_conf fills in for absent keys)."""
    return {k: v.default for k, v in inspect.signature(ECF.__init__).parameters.items()
            if v.default is not inspect.Parameter.empty}


def _check_hyper(p: dict, n_items=None, n_tags=None):
    for key in INT_KEYS:
        if isinstance(p[key], bool) or not isinstance(p[key], (int, np.integer)):
            raise ValueError(f'ECF {key} must be an int, got {p[key]!r}')
    if p['embedding_dim'] < 1:
        raise ValueError(f"ECF embedding_dim must be positive, got {p['embedding_dim']}")
    most = hip_ops.ECF_MAX_CLUSTERS if n_items is None else min(hip_ops.ECF_MAX_CLUSTERS, n_items)
    if not 1 <= p['n_clusters'] <= most:
        raise ValueError(f"ECF n_clusters must be in [1, {most}] (one wavefront lane per cluster, seeded from distinct "
                         f"items), got {p['n_clusters']}")
    for key in ('top_n', 'top_m'):
        if not 1 <= p[key] <= p['n_clusters']:
            raise ValueError(f"ECF {key} must be in [1, n_clusters = {p['n_clusters']}], got {p[key]}")
    if p['top_p'] < 1 or (n_tags is not None and p['top_p'] > n_tags):
        raise ValueError(f"ECF top_p must be in [1, n_tags{'' if n_tags is None else ' = %d' % n_tags}], "
                         f"got {p['top_p']}")
    for key in TEMP_KEYS:
        if isinstance(p[key], bool) or not isinstance(p[key], (int, float, np.integer, np.floating)) or \
                not (0 < p[key] < float('inf')):
            raise ValueError(f'ECF {key} must be a positive number, got {p[key]!r}')


def validate_ecf_conf(conf: dict):
    """The ECF keys of a conf; absent ones take the constructor's defaults.  What depends on the dataset (n_clusters
    <= n_items, top_p <= n_tags) is checked by the constructor."""
    _check_hyper({**ecf_defaults(), **{k: conf[k] for k in INT_KEYS + TEMP_KEYS if k in conf}})


def _tag_factors(tag_matrix, n_items: int):
    """(indptr int64 [n_tags + 1], indices int32) of the transposed 0/1 incidence (tags x items) and the per-tag weight
    float32 [n_tags], from a dataset that carries `tag_incidence` / `tag_weight` or from the reference's weighted
    matrix incidence @ diag(w) (scipy, [n_items, n_tags])."""
    if hasattr(tag_matrix, 'tag_incidence') and hasattr(tag_matrix, 'tag_weight'):
        inc = tag_matrix.tag_incidence.tocsc(copy=True)
        inc.sum_duplicates()
        if inc.nnz and not np.all(inc.data == 1):
            raise ValueError('ECF: the tag incidence lists an (item, tag) pair more than once')
        weight = np.asarray(tag_matrix.tag_weight, np.float64)
    else:
        if not hasattr(tag_matrix, 'tocsc'):
            raise ValueError(f'ECF tag_matrix must be a scipy sparse matrix or a dataset with tag_incidence and '
                             f'tag_weight, got {type(tag_matrix).__name__}')
        inc = tag_matrix.tocsc(copy=True)
        inc.sum_duplicates()
        weight = np.zeros(inc.shape[1], np.float64)     # a tag no item carries: its column of d_c is 0 whatever w
        used = np.nonzero(np.diff(inc.indptr))[0]
        if len(used):
            lo = np.minimum.reduceat(inc.data, inc.indptr[used])
            hi = np.maximum.reduceat(inc.data, inc.indptr[used])
            if not np.array_equal(lo, hi):
                bad = int(used[np.nonzero(lo != hi)[0][0]])
                raise ValueError(f'ECF tag_matrix must be incidence @ diag(w): the stored values of column {bad} are '
                                 f'not constant')
            weight[used] = lo
    if inc.shape[0] != n_items or weight.shape != (inc.shape[1],):
        raise ValueError(f'ECF tag_matrix has shape {inc.shape} with {weight.shape[0]} weights, expected {n_items} '
                         f'rows and one weight per tag')
    inc.sort_indices()
    return inc.indptr.astype(np.int64), inc.indices.astype(np.int32), weight.astype(np.float32)


class ECF(_HipTables):
    DENSE_KEYS = ('tag_matrix', 'interaction_matrix')   # of a reference-written model.pth, if it was handed float32
    validate_conf = staticmethod(validate_ecf_conf)   # its own keys; the SGD defaults apply as for any trained model

    def __init__(self, n_users: int, n_items: int, tag_matrix, interaction_matrix, embedding_dim: int = 100,
                 n_clusters: int = 64, top_n: int = 20, top_m: int = 20, temp_masking: float = 2.,
                 temp_tags: float = 2., top_p: int = 4, lam_cf: float = .6, lam_ind: float = 1., lam_ts: float = 1.):
        super().__init__()
        self.n_users, self.n_items = n_users, n_items
        x_ptr, x_idx, rows, cols = csr_arrays(interaction_matrix)
        if (rows, cols) != (n_users, n_items):
            raise ValueError(f'ECF interaction_matrix has shape {(rows, cols)}, expected {(n_users, n_items)}')
        t_ptr, t_idx, weight = _tag_factors(tag_matrix, n_items)
        self.n_tags = len(weight)
        _check_hyper(dict(embedding_dim=embedding_dim, n_clusters=n_clusters, top_n=top_n, top_m=top_m, top_p=top_p,
                          temp_masking=temp_masking, temp_tags=temp_tags), n_items, self.n_tags)
        self.embedding_dim, self.n_clusters = int(embedding_dim), int(n_clusters)
        self.top_n, self.top_m, self.top_p = int(top_n), int(top_m), int(top_p)
        self.temp_masking, self.temp_tags = float(temp_masking), float(temp_tags)
        self.lam_cf, self.lam_ind, self.lam_ts = lam_cf, lam_ind, lam_ts

        # construction order = the reference's (users, items, the permutation that seeds the clusters from item rows)
        self.user_embed = nn.Embedding(self.n_users, self.embedding_dim)
        self.item_embed = nn.Embedding(self.n_items, self.embedding_dim)
        indxs = torch.randperm(self.n_items)[:self.n_clusters]
        self.clusters = nn.Parameter(self.item_embed.weight[indxs].detach(), requires_grad=True)

        # the train matrix by rows, the tag incidence by tags, the tag weights: not part of the state dict, follow
        # .to(device)
        self.register_buffer('x_indptr', torch.from_numpy(x_ptr), persistent=False)
        self.register_buffer('x_indices', torch.from_numpy(x_idx), persistent=False)
        self.register_buffer('tag_indptr', torch.from_numpy(t_ptr), persistent=False)
        self.register_buffer('tag_indices', torch.from_numpy(t_idx), persistent=False)
        self.register_buffer('tag_weight', torch.from_numpy(weight), persistent=False)
        self.register_buffer('tag_rows', torch.arange(self.n_tags), persistent=False)
        self._register_load_state_dict_pre_hook(self._drop_dense_matrices)

        self._acc_ts = self._acc_ind = self._acc_cf = 0
        self._x_tildes = self._xs = None     # set by get_item_representations, read by get_user_representations
        self.name = 'ECF'
        logging.info('Built %s (HIP affiliation, sparse products): %d users, %d items, %d tags, dim %d, %d clusters, '
                     'top_n %d, top_m %d, top_p %d, temp_masking %g, temp_tags %g, lam_cf %g', self.name, n_users,
                     n_items, self.n_tags, self.embedding_dim, self.n_clusters, self.top_n, self.top_m, self.top_p,
                     self.temp_masking, self.temp_tags, self.lam_cf)

    # ------------------------------------------------------------------ persistence
    def _drop_dense_matrices(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                             error_msgs):
        """A reference-written state dict may carry its two dense matrices: shape-checked and dropped."""
        for key, shape in ((prefix + self.DENSE_KEYS[0], (self.n_items, self.n_tags)),
                           (prefix + self.DENSE_KEYS[1], (self.n_users, self.n_items))):
            if key not in state_dict:
                continue
            dense = state_dict.pop(key)
            if tuple(dense.shape) != shape:
                raise ValueError(f'{key} of the state dict has shape {tuple(dense.shape)}, this model was built on '
                                 f'{shape}')

    def load_model_from_path(self, path: str):
        """Non-strict, as the reference's (sgd_alg.py:771-775)."""
        device = next(self.parameters()).device
        self.load_state_dict(torch.load(os.path.join(path, 'model.pth'), map_location=device), strict=False)
        logging.info('Model Loaded')

    # ------------------------------------------------------------------ plugin surface
    def _generate_item_representations(self):
        self._x_tildes = cosine_to(self.item_embed.weight, self.clusters, 0., -1., 1.)      # [n_items, n_clusters]
        self._xs = hip_ops.ecf_affiliation(self._x_tildes, self.top_m, self.temp_masking)

    def get_item_representations(self, i_idxs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Regenerates the affiliations of all items: call it before get_user_representations."""
        self._generate_item_representations()
        i_embed = self.lookup(self.item_embed, i_idxs)
        x_i = hip_ops.embedding(self._xs, i_idxs, self.status_word())
        return x_i, i_embed

    def get_user_representations(self, u_idxs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._x_tildes is None:
            raise RuntimeError('ECF: get_item_representations must run before get_user_representations')
        u_embed = self.lookup(self.user_embed, u_idxs)
        a_tilde = hip_ops.sparse_rows_sum(self._x_tildes, (self.x_indptr, self.x_indices), u_idxs, self.status_word())
        a_i = hip_ops.ecf_affiliation(a_tilde, self.top_n, self.temp_masking)
        return a_i, u_embed

    def combine_user_item_representations(self, u_repr, i_repr) -> torch.Tensor:
        return _pairwise_dot(u_repr[0], i_repr[0])

    def forward(self, u_idxs: torch.Tensor, i_idxs: torch.Tensor) -> torch.Tensor:
        i_repr = self.get_item_representations(i_idxs)
        u_repr = self.get_user_representations(u_idxs)
        dots = self.combine_user_item_representations(u_repr, i_repr)

        # tag similarity: d_c [n_clusters, n_tags] = xs.T @ (incidence @ diag(w)), held transposed; the top_p tags of
        # each cluster should carry its whole softmax
        tag_sums = hip_ops.sparse_rows_sum(self._xs, (self.tag_indptr, self.tag_indices), self.tag_rows,
                                           self.status_word())
        log_b_c = torch.log_softmax(self.tag_weight[:, None] * tag_sums / self.temp_tags, dim=0)
        self._acc_ts = self._acc_ts + (-log_b_c.topk(self.top_p, dim=0).values).sum()

        # independence: every cluster closest to itself
        sim_mtx = cosine_to(self.clusters, self.clusters, 0., -1., 1.)
        self._acc_ind = self._acc_ind + torch.diag(-torch.log_softmax(sim_mtx, dim=-1)).sum()

        # BPR on the plain embeddings
        logits = _pairwise_dot(u_repr[1], i_repr[1])
        diff_logits = (logits[:, :1] - logits[:, 1:]).flatten()
        self._acc_cf = self._acc_cf + F.binary_cross_entropy_with_logits(diff_logits, torch.ones_like(diff_logits))
        return dots

    def get_and_reset_other_loss(self) -> Dict:
        acc_ts, acc_ind, acc_cf = self._acc_ts, self._acc_ind, self._acc_cf
        self._acc_ts = self._acc_ind = self._acc_cf = 0
        cf_loss, ind_loss, ts_loss = self.lam_cf * acc_cf, self.lam_ind * acc_ind, self.lam_ts * acc_ts
        return {'reg_loss': ts_loss + ind_loss + cf_loss, 'cf_loss': cf_loss, 'ind_loss': ind_loss, 'ts_loss': ts_loss}

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        """`dataset` is an ECFTrainRecDataset: the TRAIN split with the tag matrix."""
        p = {**ecf_defaults(), **conf}
        matrix = getattr(dataset, 'sampling_csr', None)
        if matrix is None:
            matrix = dataset.sampling_matrix
        tags = dataset if hasattr(dataset, 'tag_incidence') else dataset.tag_matrix
        return ECF(dataset.n_users, dataset.n_items, tags, matrix, p['embedding_dim'], p['n_clusters'], p['top_n'],
                   p['top_m'], p['temp_masking'], p['temp_tags'], p['top_p'], p['lam_cf'], p['lam_ind'], p['lam_ts'])
