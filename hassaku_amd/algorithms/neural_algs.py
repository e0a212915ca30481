"""DeepMatrixFactorization on a sparse first layer -- algorithms/sgd_alg.py:778-880 of the reference (Xue et al.,
"Deep Matrix Factorization Models for Recommender Systems", IJCAI 2017).

Two towers of nn.Linear / ReLU map a user's row and an item's column of the 0/1 train matrix to `final_dimension`
numbers; the score is their cosine, raised to mu = 1e-6 where it is smaller.  The reference feeds the towers from two
frozen dense copies of the matrix ([U, I] and [I, U] fp32 "embeddings").  Here the model holds the CSR of X and of X^T
and the first layer of each tower is the gather-sum `hip_ops.sparse_rows_sum` over a row's stored entries (stored
entries count as 1), with that layer's weight kept transposed, [n_in, H], so the kernel reads contiguous rows; its bias
is added by torch.  No U x I array exists at any time.  Everything behind the first layer -- mid layers of width
16..128, the ReLUs, the cosine -- is dense algebra on [rows, <= 128] and runs on the library path, as in proto_alg.py.

Same constructor, `u_layers` / `i_layers`, `build_from_conf` keys, RNG consumption at construction (so the same seed
gives the reference's initial towers bit for bit) and state_dict() keys and shapes (`user_nn.0.weight` [H, n_items],
...) as the reference's class: the transposed first layer is translated when a state dict is written or read.  A
model.pth written here leaves out the reference's two dense `user_vectors.weight` / `item_vectors.weight` entries (its
strict loader needs them added back: the dense train matrix and its transpose); one written by the reference loads
here, the two entries are checked against X and dropped.
"""
import logging
from typing import List, Union

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from hassaku_amd import hip_ops
from hassaku_amd.algorithms.base_classes import csr_arrays, csr_transpose
from hassaku_amd.algorithms.proto_alg import _HipTables
from hassaku_amd.train.utils import general_weight_init

COSINE_EPS = 1e-8   # nn.CosineSimilarity's default


def _layer_sizes(value, name: str) -> List[int]:
    """A conf / constructor layer spec as a list of positive ints (an int is one layer; [] is no mid layer)."""
    sizes = [value] if not isinstance(value, (list, tuple)) else list(value)
    for s in sizes:
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)):
            raise ValueError(f'DeepMatrixFactorization {name} must be a positive int or a list of them, '
                             f'got {value!r}')
        if s <= 0:
            raise ValueError(f'DeepMatrixFactorization {name} must be positive, got {value!r}')
    return [int(s) for s in sizes]


def validate_dmf_conf(conf: dict):
    """The DMF keys of a conf (sgd_alg.py:859-862): all three required, as the reference's build_from_conf reads them."""
    for key in ('u_mid_layers', 'i_mid_layers', 'final_dimension'):
        if key not in conf:
            raise ValueError(f'DeepMatrixFactorization conf needs {key}')
    _layer_sizes(conf['u_mid_layers'], 'u_mid_layers')
    _layer_sizes(conf['i_mid_layers'], 'i_mid_layers')
    if isinstance(conf['final_dimension'], (list, tuple)):
        raise ValueError(f"DeepMatrixFactorization final_dimension must be a positive int, "
                         f"got {conf['final_dimension']!r}")
    _layer_sizes(conf['final_dimension'], 'final_dimension')


class SparseInputLinear(nn.Module):
    """nn.Linear(n_in, n_out) whose input is a 0/1 row of a CSR: `weight_t` [n_in, n_out] is the weight transposed.
    In a state dict it appears as nn.Linear does: `weight` [n_out, n_in] and `bias` [n_out]."""

    def __init__(self, linear: nn.Linear):
        super().__init__()
        self.in_features, self.out_features = linear.in_features, linear.out_features
        self.weight_t = nn.Parameter(linear.weight.detach().t().contiguous())
        self.bias = nn.Parameter(linear.bias.detach().clone())

    def forward(self, csr, idx: torch.Tensor, status=None) -> torch.Tensor:
        return hip_ops.sparse_rows_sum(self.weight_t, csr, idx, status) + self.bias

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        w, b = self.weight_t.t().contiguous(), self.bias
        destination[prefix + 'weight'] = w if keep_vars else w.detach()
        destination[prefix + 'bias'] = b if keep_vars else b.detach()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        for key, param, shape in ((prefix + 'weight', self.weight_t, (self.out_features, self.in_features)),
                                  (prefix + 'bias', self.bias, (self.out_features,))):
            if key not in state_dict:
                if strict:
                    missing_keys.append(key)
                continue
            value = state_dict[key]
            if tuple(value.shape) != shape:
                error_msgs.append(f'size mismatch for {key}: copying a param with shape {tuple(value.shape)} from '
                                  f'checkpoint, the shape in current model is {shape}.')
                continue
            with torch.no_grad():
                param.copy_(value.t() if value.dim() == 2 else value)

    def extra_repr(self) -> str:
        return f'in_features={self.in_features}, out_features={self.out_features}, sparse 0/1 input'


def _tower(layers: List[int]) -> nn.Sequential:
    mods = []
    for k, (n_in, n_out) in enumerate(zip(layers[:-1], layers[1:])):
        mods.append(nn.Linear(n_in, n_out))
        if k != len(layers) - 2:
            mods.append(nn.ReLU())
    return nn.Sequential(*mods)


class DeepMatrixFactorization(_HipTables):
    DENSE_KEYS = ('user_vectors.weight', 'item_vectors.weight')   # of a reference-written model.pth
    validate_conf = staticmethod(validate_dmf_conf)   # its own keys; the SGD defaults apply as for any trained model

    def __init__(self, matrix, u_mid_layers: Union[List[int], int], i_mid_layers: Union[List[int], int],
                 final_dimension: int):
        super().__init__()
        indptr, indices, self.n_users, self.n_items = csr_arrays(matrix)
        self.mu = 1.e-6   # equation (13) of the paper
        self.final_dimension = _layer_sizes(final_dimension, 'final_dimension')[0]
        if isinstance(final_dimension, (list, tuple)):
            raise ValueError(f'DeepMatrixFactorization final_dimension must be a positive int, got {final_dimension!r}')
        self.u_layers = [self.n_items] + _layer_sizes(u_mid_layers, 'u_mid_layers') + [self.final_dimension]
        self.i_layers = [self.n_users] + _layer_sizes(i_mid_layers, 'i_mid_layers') + [self.final_dimension]
        for side, layers in (('user', self.u_layers), ('item', self.i_layers)):
            width, limit = layers[1], hip_ops.sparse_rows_max_dim(layers[1])
            if width > limit:
                raise ValueError(f'DeepMatrixFactorization: the first hidden width of the {side} tower is {width}; the '
                                 f'sparse first layer serves at most {limit} for a width with this alignment (2048 if '
                                 f'a multiple of 4, 1024 if even, 512 if odd)')
        # construction order = the reference's: both towers with nn.Linear's own init (user first), then
        # general_weight_init over the user tower and over the item tower -- same seed, same initial towers
        self.user_nn = _tower(self.u_layers)
        self.item_nn = _tower(self.i_layers)
        self.user_nn.apply(general_weight_init)
        self.item_nn.apply(general_weight_init)
        self.user_nn[0] = SparseInputLinear(self.user_nn[0])
        self.item_nn[0] = SparseInputLinear(self.item_nn[0])

        x_ptr, x_idx = torch.from_numpy(indptr), torch.from_numpy(indices)
        t_ptr, t_idx, _ = csr_transpose(x_ptr, x_idx, None, self.n_users, self.n_items)
        # the train matrix by rows (users) and by columns (items); not part of the state dict, follow .to(device)
        self.register_buffer('x_indptr', x_ptr, persistent=False)
        self.register_buffer('x_indices', x_idx, persistent=False)
        self.register_buffer('t_indptr', t_ptr, persistent=False)
        self.register_buffer('t_indices', t_idx, persistent=False)
        self._register_load_state_dict_pre_hook(self._drop_dense_vectors)

        self.name = 'DeepMatrixFactorization'
        logging.info('Built %s (HIP sparse first layer) \n- u_layers: %s \n- i_layers: %s \n', self.name, self.u_layers,
                     self.i_layers)

    # ------------------------------------------------------------------ persistence
    def _drop_dense_vectors(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                            error_msgs):
        """A reference-written state dict also carries the dense train matrix and its transpose: checked against X
        (shape, then entry by entry: as many non-zeros as X stores, and a 1 at each of them) and dropped."""
        rows = torch.repeat_interleave(torch.arange(self.n_users), (self.x_indptr[1:] - self.x_indptr[:-1]).cpu())
        cols = self.x_indices.cpu().long()
        for key, shape, at in ((prefix + self.DENSE_KEYS[0], (self.n_users, self.n_items), (rows, cols)),
                               (prefix + self.DENSE_KEYS[1], (self.n_items, self.n_users), (cols, rows))):
            if key not in state_dict:
                continue
            dense = state_dict.pop(key)
            if tuple(dense.shape) != shape:
                raise ValueError(f'{key} of the state dict has shape {tuple(dense.shape)}, the train matrix gives '
                                 f'{shape}')
            dense = dense.detach().cpu()
            if int(torch.count_nonzero(dense)) != len(cols) or not bool((dense[at] == 1).all()):
                raise ValueError(f'{key} of the state dict is not the train matrix this model was built on')

    # ------------------------------------------------------------------ plugin surface
    def _run_tower(self, tower: nn.Sequential, csr, idx: torch.Tensor) -> torch.Tensor:
        h = tower[0](csr, idx, self.status_word())
        for layer in list(tower)[1:]:
            h = layer(h)
        return h

    def get_user_representations(self, u_idxs: torch.Tensor) -> torch.Tensor:
        return self._run_tower(self.user_nn, (self.x_indptr, self.x_indices), u_idxs)

    def get_item_representations(self, i_idxs: torch.Tensor) -> torch.Tensor:
        return self._run_tower(self.item_nn, (self.t_indptr, self.t_indices), i_idxs)

    def combine_user_item_representations(self, u_repr: torch.Tensor, i_repr: torch.Tensor) -> torch.Tensor:
        """Cosine of u_repr [B, F] with i_repr [B, K, F] -> [B, K], or with a shared item list i_repr [I, F] -> [B, I]
        (evaluation); values below mu are set to mu and pass no gradient (the reference's masked assignment)."""
        if i_repr.dim() == 2:
            # nn.CosineSimilarity's arithmetic, x / max(|x|, eps) on each side, without a [B, I, F] product
            u = u_repr / u_repr.norm(dim=-1, keepdim=True).clamp_min(COSINE_EPS)
            i = i_repr / i_repr.norm(dim=-1, keepdim=True).clamp_min(COSINE_EPS)
            sim = u @ i.T
        else:
            sim = F.cosine_similarity(u_repr[:, None, :], i_repr, dim=-1, eps=COSINE_EPS)
        return torch.where(sim < self.mu, torch.full_like(sim, self.mu), sim)

    @staticmethod
    def build_from_conf(conf: dict, train_dataset):
        """`train_dataset` is the TRAIN split's dataset: the towers read the train matrix."""
        matrix = getattr(train_dataset, 'sampling_csr', None)
        if matrix is None:
            matrix = train_dataset.iteration_matrix
        return DeepMatrixFactorization(matrix, conf['u_mid_layers'], conf['i_mid_layers'], conf['final_dimension'])
