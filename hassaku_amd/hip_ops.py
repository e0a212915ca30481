"""Thin torch-tensor front end over the C ABI (include/hassaku_hip.h).

PyTorch is used here only as the owner of device memory and streams; every computation is a HIP
kernel of libhassaku_hip.so.  Shapes are validated on the host before any pointer is handed over.
"""
import ctypes
from typing import Optional, Sequence, Tuple

import torch

from hassaku_amd import _lib
from hassaku_amd._lib import HskBprmfState

ADAM_BETA1, ADAM_BETA2, ADAM_EPS = 0.9, 0.999, 1e-8  # torch.optim.AdamW defaults (train/trainer.py:52-53)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk(t: Optional[torch.Tensor], dtype, name: str, shape: Optional[Tuple[int, ...]] = None, optional=False):
    if t is None:
        if optional:
            return
        raise ValueError(f'{name} must not be None')
    if not t.is_cuda:
        raise RuntimeError(f'{name} must live on the HIP device (got {t.device}); there is no CPU path')
    if t.dtype != dtype:
        raise TypeError(f'{name} must be {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise ValueError(f'{name} must be contiguous')
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name} has shape {tuple(t.shape)}, expected {tuple(shape)}')


def _chk_gram(t: torch.Tensor, name: str) -> Tuple[int, int]:
    """(n, ld) of a contiguous fp64 matrix [n, ld >= n] on the device: a square matrix in its first n columns."""
    _chk(t, torch.float64, name)
    if t.dim() != 2 or t.shape[1] < t.shape[0]:
        raise ValueError(f'{name} has shape {tuple(t.shape)}, expected [n, ld >= n]')
    return t.shape[0], t.shape[1]


def new_status(device) -> torch.Tensor:
    return torch.zeros(1, dtype=torch.int32, device=device)


def raise_on_status(status: torch.Tensor, what: str = ''):
    """Synchronising check of the device status word."""
    s = int(status.item())
    if s & 1:
        raise IndexError(f'{what}: index out of range in self')
    if s & 2:
        raise RuntimeError(f'{what}: negative sampler gave up (a user interacted with ~every item)')


def check_and_clear_status(status: Optional[torch.Tensor], what: str = ''):
    """raise_on_status for a word that outlives the check (a model's): what it has seen "since the last check".  A set
    word is cleared BEFORE the raise -- left set, it would fail every later check of a model that has seen one bad
    index.  One host sync when the word is clear; a read that fails itself leaves the word alone."""
    if status is None or int(status.item()) == 0:
        return
    seen = status.clone()
    status.zero_()
    raise_on_status(seen, what)


# ------------------------------------------------------------------------------------------------
# un-fused operators
# ------------------------------------------------------------------------------------------------
def mf_scores(user_emb, item_emb, item_bias, user_bias, global_bias, u_idx, i_idx, status=None):
    """logits[b,k] = <U[u_b], I[i_bk]> + biases.  u_idx [B] int64, i_idx [B,K] int64 -> [B,K] fp32."""
    _lib.require_gpu()
    lib = _lib.load()
    n_users, dim = user_emb.shape
    n_items = item_emb.shape[0]
    _chk(user_emb, torch.float32, 'user_emb')
    _chk(item_emb, torch.float32, 'item_emb', (n_items, dim))
    _chk(item_bias, torch.float32, 'item_bias', optional=True)
    _chk(user_bias, torch.float32, 'user_bias', optional=True)
    _chk(global_bias, torch.float32, 'global_bias', optional=True)
    if item_bias is not None and item_bias.numel() != n_items:
        raise ValueError('item_bias size mismatch')
    if user_bias is not None and user_bias.numel() != n_users:
        raise ValueError('user_bias size mismatch')
    _chk(u_idx, torch.int64, 'u_idx')
    _chk(i_idx, torch.int64, 'i_idx')
    if u_idx.dim() != 1 or i_idx.dim() != 2 or i_idx.shape[0] != u_idx.shape[0]:
        raise ValueError(f'u_idx {tuple(u_idx.shape)} / i_idx {tuple(i_idx.shape)}: expected [B] and [B,K]')
    B, K = i_idx.shape
    out = torch.empty((B, K), dtype=torch.float32, device=user_emb.device)
    # the kernel takes at most 65535 rows per launch
    for lo in range(0, B, 65535):
        hi = min(B, lo + 65535)
        _lib.check(lib.hsk_mf_scores(_p(user_emb), _p(item_emb), _p(item_bias), _p(user_bias), _p(global_bias),
                                     n_users, n_items, dim, _p(u_idx[lo:hi]), _p(i_idx[lo:hi]), hi - lo, K,
                                     _p(out[lo:hi]), _p(status), _stream()), 'hsk_mf_scores')
    return out


def bpr_loss_grad(logits: torch.Tensor, need_grad: bool = True):
    """-> (loss fp64 [1], grad_logits fp32 [B,K] or None)."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(logits, torch.float32, 'logits')
    if logits.dim() != 2 or logits.shape[1] < 2 or logits.shape[0] < 1:
        raise ValueError(f'logits must be [B>=1, K>=2], got {tuple(logits.shape)}')
    B, K = logits.shape
    loss = torch.empty(1, dtype=torch.float64, device=logits.device)
    ws = torch.empty(B, dtype=torch.float64, device=logits.device)
    grad = torch.empty_like(logits) if need_grad else None
    _lib.check(lib.hsk_bpr_loss_grad(_p(logits), B, K, _p(loss), _p(grad), _p(ws), _stream()), 'hsk_bpr_loss_grad')
    return loss, grad


LOSS_KINDS = {'bpr': 0, 'bce': 1, 'sampled_softmax': 2}   # HSK_LOSS_* of include/hassaku_hip.h


def rec_loss_grad(kind: str, logits: torch.Tensor, log_adjust: float = 0.0, need_grad: bool = True):
    """Any of the reference's three losses on logits [B, 1+N] -> (loss fp64 [1], grad_logits fp32 [B,K] or None)."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(logits, torch.float32, 'logits')
    if logits.dim() != 2 or logits.shape[1] < 2 or logits.shape[0] < 1:
        raise ValueError(f'logits must be [B>=1, K>=2], got {tuple(logits.shape)}')
    B, K = logits.shape
    loss = torch.empty(1, dtype=torch.float64, device=logits.device)
    ws = torch.empty(B, dtype=torch.float64, device=logits.device)
    grad = torch.empty_like(logits) if need_grad else None
    _lib.check(lib.hsk_rec_loss_grad(LOSS_KINDS[kind], _p(logits), B, K, float(log_adjust), _p(loss), _p(grad), _p(ws),
                                     _stream()), 'hsk_rec_loss_grad')
    return loss, grad


def mf_backward(user_emb, item_emb, u_idx, i_idx, grad_logits, want_item_bias, want_user_bias, want_global_bias,
                status=None):
    """Dense parameter gradients (what embedding_dense_backward would give)."""
    _lib.require_gpu()
    lib = _lib.load()
    n_users, dim = user_emb.shape
    n_items = item_emb.shape[0]
    _chk(user_emb, torch.float32, 'user_emb')
    _chk(item_emb, torch.float32, 'item_emb', (n_items, dim))
    _chk(u_idx, torch.int64, 'u_idx')
    _chk(i_idx, torch.int64, 'i_idx')
    B, K = i_idx.shape
    _chk(grad_logits, torch.float32, 'grad_logits', (B, K))
    if u_idx.shape != (B,):
        raise ValueError('u_idx / i_idx batch mismatch')
    if B > 65535:
        raise ValueError('mf_backward handles at most 65535 rows per call')
    dev = user_emb.device
    g_u = torch.empty_like(user_emb)
    g_i = torch.empty_like(item_emb)
    g_ib = torch.empty(n_items, dtype=torch.float32, device=dev) if want_item_bias else None
    g_ub = torch.empty(n_users, dtype=torch.float32, device=dev) if want_user_bias else None
    g_gb = torch.empty(1, dtype=torch.float32, device=dev) if want_global_bias else None
    _lib.check(lib.hsk_mf_backward(_p(user_emb), _p(item_emb), n_users, n_items, dim, _p(u_idx), _p(i_idx), B, K,
                                   _p(grad_logits), _p(g_u), _p(g_i), _p(g_ib), _p(g_ub), _p(g_gb), _p(status),
                                   _stream()), 'hsk_mf_backward')
    return g_u, g_i, g_ib, g_ub, g_gb


def bias_scores(item_bias, user_bias, global_bias, u_idx, i_idx, status=None):
    """Bias-only model (SGDBaseline, algorithms/sgd_alg.py:72-107): logits[b,k] = ub[u_b] + ib[i_bk] + gb."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(item_bias, torch.float32, 'item_bias')
    _chk(user_bias, torch.float32, 'user_bias')
    _chk(global_bias, torch.float32, 'global_bias', optional=True)
    _chk(u_idx, torch.int64, 'u_idx')
    _chk(i_idx, torch.int64, 'i_idx')
    if u_idx.dim() != 1 or i_idx.dim() != 2 or i_idx.shape[0] != u_idx.shape[0]:
        raise ValueError(f'u_idx {tuple(u_idx.shape)} / i_idx {tuple(i_idx.shape)}: expected [B] and [B,K]')
    B, K = i_idx.shape
    out = torch.empty((B, K), dtype=torch.float32, device=item_bias.device)
    for lo in range(0, B, 65535):
        hi = min(B, lo + 65535)
        _lib.check(lib.hsk_mf_scores(None, None, _p(item_bias), _p(user_bias), _p(global_bias), user_bias.numel(),
                                     item_bias.numel(), 0, _p(u_idx[lo:hi]), _p(i_idx[lo:hi]), hi - lo, K,
                                     _p(out[lo:hi]), _p(status), _stream()), 'hsk_mf_scores')
    return out


def bias_backward(n_users, n_items, u_idx, i_idx, grad_logits, want_global_bias=True, status=None):
    """Dense gradients of the bias-only model -> (g_item_bias [I], g_user_bias [U], g_global_bias [1] | None)."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(u_idx, torch.int64, 'u_idx')
    _chk(i_idx, torch.int64, 'i_idx')
    B, K = i_idx.shape
    _chk(grad_logits, torch.float32, 'grad_logits', (B, K))
    if B > 65535:
        raise ValueError('bias_backward handles at most 65535 rows per call')
    dev = grad_logits.device
    g_ib = torch.empty(n_items, dtype=torch.float32, device=dev)
    g_ub = torch.empty(n_users, dtype=torch.float32, device=dev)
    g_gb = torch.empty(1, dtype=torch.float32, device=dev) if want_global_bias else None
    _lib.check(lib.hsk_mf_backward(None, None, n_users, n_items, 0, _p(u_idx), _p(i_idx), B, K, _p(grad_logits), None,
                                   None, _p(g_ib), _p(g_ub), _p(g_gb), _p(status), _stream()), 'hsk_mf_backward')
    return g_ib, g_ub, g_gb


class _Embedding(torch.autograd.Function):
    """rows = table[idx] through hsk_embedding_gather; backward = hsk_embedding_backward (dense gradient, duplicates
    summed in ascending position -- nn.Embedding(sparse=False) semantics, deterministic)."""

    @staticmethod
    def forward(ctx, table, idx, status):
        _lib.require_gpu()
        lib = _lib.load()
        _chk(table, torch.float32, 'embedding table')
        _chk(idx, torch.int64, 'embedding indices')
        n_rows, dim = table.shape
        flat = idx.reshape(-1)
        out = torch.empty((flat.numel(), dim), dtype=torch.float32, device=table.device)
        _lib.check(lib.hsk_embedding_gather(_p(table), n_rows, dim, _p(flat), flat.numel(), _p(out), _p(status),
                                            _stream()), 'hsk_embedding_gather')
        ctx.save_for_backward(flat)
        ctx.shape, ctx.status = (n_rows, dim), status
        return out.view(tuple(idx.shape) + (dim,))

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        (flat,) = ctx.saved_tensors
        n_rows, dim = ctx.shape
        g = grad_out.reshape(-1, dim).contiguous()
        grad_table = torch.empty((n_rows, dim), dtype=torch.float32, device=g.device)
        if flat.numel() == 0:
            return grad_table.zero_(), None, None
        nbytes = lib.hsk_embedding_backward_ws_bytes(n_rows, flat.numel())
        if nbytes <= 0:
            raise ValueError('embedding table too large for the deterministic index sort')
        ws = torch.empty(nbytes, dtype=torch.uint8, device=g.device)
        _lib.check(lib.hsk_embedding_backward(_p(g), _p(flat), flat.numel(), n_rows, dim, _p(grad_table), _p(ws), nbytes,
                                              _p(ctx.status), _stream()), 'hsk_embedding_backward')
        return grad_table, None, None


def embedding(table: torch.Tensor, idx: torch.Tensor, status=None) -> torch.Tensor:
    """table[idx] -> idx.shape + (dim,), differentiable wrt `table` (dense gradient)."""
    return _Embedding.apply(table, idx.contiguous(), status)


SORT_KINDS = ('unsupported', 'lds', 'small2', 'small4', 'small8', 'two_level')   # hsk_key_sort_plan's return value


def key_sort_plan(n_keys: int, n_entries: int, touched: bool = False) -> dict:
    """Which of the three sorts of csrc/hsk_sort.h `n_entries` entries over `n_keys` keys take, and with what (debug /
    parity; host arithmetic, no device): {'kind': one of SORT_KINDS, 'shift', 'n_buckets', 'ipb', 'epw', 'n_units' (the
    two-level plan, else 0), 'lds_bytes' (dynamic LDS of the launch), 'nbits' (radix bits of the block radix sort)}."""
    out = (ctypes.c_int64 * 8)()
    kind = _lib.load().hsk_key_sort_plan(int(n_keys), int(n_entries), int(bool(touched)), out)
    plan = dict(zip(('kind', 'shift', 'n_buckets', 'ipb', 'epw', 'n_units', 'lds_bytes', 'nbits'), (int(v) for v in out)))
    plan['kind'] = SORT_KINDS[kind]
    return plan


def key_sort(keys: torch.Tensor, n_keys: int, touched: bool = False, n_valid=None):
    """The stable sort of positions by key, as the step and the operators' backward passes run it (debug / parity).
    keys int64 [n] in [0, n_keys) -> (perm int32 [n], offsets int32 [n_keys + 1]), with touched=True also (touched
    int32 [n], n_touched int32 [1]): the keys that have entries, in any order.  n_valid (int, or device int32 [1]):
    only the first n_valid positions are entries -- perm is then defined up to offsets[n_keys] == n_valid."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(keys, torch.int64, 'keys')
    if n_valid is not None and not torch.is_tensor(n_valid):   # a host number: the count still reaches the sort on the device
        n_valid = torch.tensor([int(n_valid)], dtype=torch.int32, device=keys.device)
    _chk(n_valid, torch.int32, 'n_valid', (1,), optional=True)
    n = keys.numel()
    if keys.dim() != 1 or n < 1 or n_keys < 1:
        raise ValueError(f'keys {tuple(keys.shape)} / n_keys {n_keys}: expected [n >= 1] and n_keys >= 1')
    nbytes = lib.hsk_key_sort_ws_bytes(n_keys, n, int(bool(touched)))
    if nbytes <= 0:
        raise ValueError(f'n_keys {n_keys} too large for the item sort' + (' with a touched list' if touched else ''))
    dev_ = keys.device
    # the sort leaves its results in the workspace: poisoned (0xA5A5A5A5 is no position, offset or key), so that a word
    # a kernel fails to write shows, whatever an earlier call of the same shape left in the allocator's block
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev_)
    perm = torch.full((n,), -1, dtype=torch.int32, device=dev_)
    offsets = torch.full((n_keys + 1,), -1, dtype=torch.int32, device=dev_)
    tl = torch.full((n,), -1, dtype=torch.int32, device=dev_) if touched else None
    tn = torch.full((1,), -1, dtype=torch.int32, device=dev_) if touched else None
    status = new_status(dev_)
    _lib.check(lib.hsk_key_sort(_p(keys), n, n_keys, _p(n_valid), _p(perm), _p(offsets), _p(tl), _p(tn), _p(ws), nbytes,
                                _p(status), _stream()), 'hsk_key_sort')
    raise_on_status(status, 'key_sort')
    return (perm, offsets, tl, tn) if touched else (perm, offsets)


SPARSE_ROWS_MAX_DIM = {0: 2048, 2: 1024, 1: 512, 3: 512}   # dim % 4 -> widest row hsk_dispatch_dim serves: 64 V 8


def sparse_rows_max_dim(dim: int) -> int:
    """The widest `dim` with dim's alignment that hsk_sparse_rows_sum serves (hsk_dispatch_dim's limit)."""
    return SPARSE_ROWS_MAX_DIM[dim % 4]


class _SparseRowsSum(torch.autograd.Function):
    """out[j] = sum of Wt[c] over the stored entries c of CSR row idx[j] (hsk_sparse_rows_sum): a 0/1 row times a
    linear layer whose weight is kept transposed.  backward = hsk_sparse_rows_sum_backward: dense gradient of Wt, terms
    added in ascending position, deterministic.  One host read-back (the batch's entry count) per backward."""

    @staticmethod
    def forward(ctx, Wt, indptr, indices, idx, status):
        _lib.require_gpu()
        lib = _lib.load()
        _chk(Wt, torch.float32, 'Wt')
        if Wt.dim() != 2:
            raise ValueError(f'Wt has shape {tuple(Wt.shape)}, expected [n_in, dim]')
        n_rows = indptr.numel() - 1
        _chk(indptr, torch.int64, 'indptr', (n_rows + 1,))
        _chk(indices, torch.int32, 'indices')
        _chk(idx, torch.int64, 'row indices')
        if n_rows < 1:
            raise ValueError('the CSR has no rows')
        n_in, dim = Wt.shape
        flat = idx.reshape(-1)
        out = torch.empty((flat.numel(), dim), dtype=torch.float32, device=Wt.device)
        _lib.check(lib.hsk_sparse_rows_sum(_p(Wt), n_in, dim, _p(indptr), _p(indices), n_rows, _p(flat), flat.numel(),
                                           _p(out), _p(status), _stream()), 'hsk_sparse_rows_sum')
        ctx.save_for_backward(indptr, indices, flat)
        ctx.shape, ctx.status = (n_in, dim, n_rows), status
        return out.view(tuple(idx.shape) + (dim,))

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        indptr, indices, flat = ctx.saved_tensors
        n_in, dim, n_rows = ctx.shape
        n = flat.numel()
        g = grad_out.reshape(-1, dim).contiguous()
        grad_Wt = torch.empty((n_in, dim), dtype=torch.float32, device=g.device)
        pair_off, n_pairs = None, 0
        if n:
            pair_off = torch.empty(n + 1, dtype=torch.int64, device=g.device)
            _lib.check(lib.hsk_sparse_rows_offsets(_p(indptr), n_rows, _p(flat), n, _p(pair_off), _p(ctx.status),
                                                   _stream()), 'hsk_sparse_rows_offsets')
            n_pairs = int(pair_off[n].item())   # the one read-back: sizes the workspace
        nbytes = lib.hsk_sparse_rows_sum_backward_ws_bytes(n_in, n_pairs)
        if nbytes <= 0:
            raise ValueError(f'{n_in} input columns / {n_pairs} batch entries: too many for the deterministic sort')
        ws = torch.empty(nbytes, dtype=torch.uint8, device=g.device)
        _lib.check(lib.hsk_sparse_rows_sum_backward(_p(g), _p(indptr), _p(indices), n_rows, n_in, _p(flat), n,
                                                    _p(pair_off), n_pairs, dim, _p(grad_Wt), _p(ws), nbytes,
                                                    _p(ctx.status), _stream()), 'hsk_sparse_rows_sum_backward')
        return grad_Wt, None, None, None, None


def sparse_rows_sum(Wt: torch.Tensor, csr, idx: torch.Tensor, status=None) -> torch.Tensor:
    """X[idx] @ Wt for a 0/1 CSR X -> idx.shape + (dim,), differentiable wrt `Wt` (dense gradient).
    csr: (indptr int64 [n_rows + 1], indices int32[, n_cols]); a column id names a row of Wt [n_in, dim]."""
    indptr, indices = csr[0], csr[1]
    if len(csr) > 2 and csr[2] != Wt.shape[0]:
        raise ValueError(f'the CSR has {csr[2]} columns, Wt {Wt.shape[0]} rows')
    return _SparseRowsSum.apply(Wt, indptr, indices, idx.contiguous(), status)


ECF_MAX_CLUSTERS = 64   # one wavefront lane per taste cluster (HSK_ECF_MAX_CLUSTERS of csrc/hsk_ecf.hip)


class _EcfAffiliation(torch.autograd.Function):
    """A = sigmoid(S) * (p + (m - p)) along the rows of S [n, C], p = softmax(S / temp), m the exact top-k mask with the
    lower index winning a tie (hsk_ecf_affiliation).  backward = hsk_ecf_affiliation_backward: the gradient passes
    through p only; nothing but S is saved.  Both directions are deterministic."""

    @staticmethod
    def forward(ctx, S, top_k, temp):
        _lib.require_gpu()
        lib = _lib.load()
        _chk(S, torch.float32, 'S')
        if S.dim() != 2:
            raise ValueError(f'S has shape {tuple(S.shape)}, expected [n, n_clusters]')
        n, C = S.shape
        if not 1 <= C <= ECF_MAX_CLUSTERS:
            raise ValueError(f'S has {C} clusters per row, 1..{ECF_MAX_CLUSTERS} are served')
        if isinstance(top_k, bool) or int(top_k) != top_k or not 1 <= top_k <= C:
            raise ValueError(f'top_k must be an integer in [1, {C}], got {top_k!r}')
        temp = float(temp)
        if not (temp > 0 and temp != float('inf')):
            raise ValueError(f'the temperature must be positive and finite, got {temp!r}')
        A = torch.empty_like(S)
        _lib.check(lib.hsk_ecf_affiliation(_p(S), n, C, int(top_k), temp, _p(A), _stream()), 'hsk_ecf_affiliation')
        ctx.save_for_backward(S)
        ctx.args = (n, C, int(top_k), temp)
        return A

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        S, = ctx.saved_tensors
        n, C, top_k, temp = ctx.args
        G = grad_out.contiguous()
        _chk(G, torch.float32, 'grad of the affiliations', (n, C))
        dS = torch.empty_like(S)
        _lib.check(lib.hsk_ecf_affiliation_backward(_p(S), _p(G), n, C, top_k, temp, _p(dS), _stream()),
                   'hsk_ecf_affiliation_backward')
        return dS, None, None


def ecf_affiliation(S: torch.Tensor, top_k: int, temp: float) -> torch.Tensor:
    """Sparse affiliations [n, C] of the rows of similarities S [n, C] (fp32, contiguous, C <= ECF_MAX_CLUSTERS) to
    their top_k taste clusters; differentiable wrt S with the softmax at temperature `temp` standing in for the mask."""
    return _EcfAffiliation.apply(S, top_k, temp)


def adamw_dense(p, g, m, v, lr, wd, step, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS):
    """In-place dense AdamW step (step is 1-based)."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(p, torch.float32, 'p')
    _chk(m, torch.float32, 'm', tuple(p.shape))
    _chk(v, torch.float32, 'v', tuple(p.shape))
    _chk(g, torch.float32, 'g', tuple(p.shape), optional=True)
    _lib.check(lib.hsk_adamw_dense(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, wd, step, _stream()),
               'hsk_adamw_dense')


LAZY_USERS_MIN_ELEMENTS = 4_000_000   # user tables above this many elements are updated lazily (BprMfFusedState)
OPT_KINDS = {'adamw': 0, 'adam': 1, 'adagrad': 2}            # HSK_OPT_* (conf['optimizer'], train/trainer.py:48-53)
ADAGRAD_EPS = 1e-10                                           # torch.optim.Adagrad default


def opt_eps(optimizer: str, eps=None) -> float:
    """torch's default eps of the optimiser unless given."""
    if eps is not None:
        return eps
    return ADAGRAD_EPS if optimizer == 'adagrad' else ADAM_EPS


def opt_dense(optimizer, p, g, m, v, lr, wd, step, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=None):
    """In-place dense step of 'adamw' | 'adam' | 'adagrad' (torch.optim defaults; weight_decay = L2 for the last
    two).  v is exp_avg_sq / adagrad's state_sum; step is 1-based."""
    _lib.require_gpu()
    lib = _lib.load()
    if optimizer not in OPT_KINDS:
        raise ValueError(f'Optimizer {optimizer} not yet implemented')
    _chk(p, torch.float32, 'p')
    _chk(m, torch.float32, 'm', tuple(p.shape))
    _chk(v, torch.float32, 'v', tuple(p.shape))
    _chk(g, torch.float32, 'g', tuple(p.shape), optional=True)
    _lib.check(lib.hsk_opt_dense(OPT_KINDS[optimizer], _p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2,
                                 opt_eps(optimizer, eps), wd, step, _stream()), 'hsk_opt_dense')


def build_alias_table(p):
    """Walker/Vose alias table of a discrete distribution p (host, float64) -> (prob float32 [n], alias int32 [n]):
    draw a uniform column j, keep j with probability prob[j], else take alias[j]."""
    import numpy as np
    p = np.asarray(p, dtype=np.float64)
    n = len(p)
    if n == 0 or p.min() < 0 or not np.isfinite(p).all() or p.sum() <= 0:
        raise ValueError('alias table needs a non-empty, non-negative, finite distribution')
    scaled = p / p.sum() * n
    prob, alias = np.ones(n, dtype=np.float64), np.arange(n, dtype=np.int32)
    small = [i for i in range(n) if scaled[i] < 1.0]
    large = [i for i in range(n) if scaled[i] >= 1.0]
    while small and large:
        s, g = small.pop(), large.pop()
        prob[s], alias[s] = scaled[s], g
        scaled[g] -= 1.0 - scaled[s]
        (small if scaled[g] < 1.0 else large).append(g)
    return prob.astype(np.float32), alias


def sample_negatives_uniform(csr_indptr, csr_indices, n_items, u_idx, n_neg, seed, stream_id=0, status=None,
                             alias=None):
    """neg[b,n] ~ U{[0,n_items) minus the CSR row of u_b}  (alias=None), or the item distribution of the alias table
    (alias = (prob f32 [I], idx i32 [I]) device tensors) restricted the same way.  -> int64 [B, n_neg]."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(csr_indptr, torch.int64, 'csr_indptr')
    _chk(csr_indices, torch.int32, 'csr_indices')
    _chk(u_idx, torch.int64, 'u_idx')
    n_users = csr_indptr.numel() - 1
    B = u_idx.numel()
    out = torch.empty((B, n_neg), dtype=torch.int64, device=u_idx.device)
    if alias is None:
        _lib.check(lib.hsk_sample_negatives_uniform(_p(csr_indptr), _p(csr_indices), n_users, n_items, _p(u_idx), B,
                                                    n_neg, seed, stream_id, _p(out), _p(status), _stream()),
                   'hsk_sample_negatives_uniform')
    else:
        prob, idx = alias
        _chk(prob, torch.float32, 'alias prob', (n_items,))
        _chk(idx, torch.int32, 'alias idx', (n_items,))
        _lib.check(lib.hsk_sample_negatives_alias(_p(csr_indptr), _p(csr_indices), n_users, n_items, _p(prob), _p(idx),
                                                  _p(u_idx), B, n_neg, seed, stream_id, _p(out), _p(status),
                                                  _stream()), 'hsk_sample_negatives_alias')
    return out


# ------------------------------------------------------------------------------------------------
# fused training step
# ------------------------------------------------------------------------------------------------
class BprMfFusedState:
    """Owns the torch tensors the C `hsk_bprmf_state` points at (moments, workspace, loss, status).

    Parameters are borrowed from the model (`nn.Parameter.data`): the fused step writes into the model's own
    tensors.  With the lazy AdamW (lazy_users, the default; lazy_items on large catalogues) a row outside the batch
    keeps its pending zero-gradient steps until it is next touched or swept -- any number of them: the periodic sweep
    comes every 64 steps at most for small batches and not at all at the headline shape (flush_cadence()), where rows
    go hundreds of steps behind: call flush() before reading the tables
    (state_dict(), save_model_to_path(), evaluation) -- Trainer does.  One instance per (model, hyper-parameters).

    start_step: the optimiser's step counter before the first step (resuming a run): rows and moments are taken as
    current at that step -- preload `m[k]` / `v[k]` (the tensors the C state points at) before the first step.
    """

    def __init__(self, user_emb, item_emb, item_bias=None, user_bias=None, global_bias=None, *, lr, wd,
                 max_batch, max_cols, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=None, seed=0,
                 csr_indptr=None, csr_indices=None, coo_user=None, coo_item=None, lazy_users='auto', overlap=True,
                 loss='bpr', log_adjust=0.0, alias=None, optimizer='adamw', lazy_items='auto', graph_chunk=0,
                 flush_every=0, start_step=0):
        _lib.require_gpu()
        if optimizer not in OPT_KINDS:
            raise ValueError(f'Optimizer {optimizer} not yet implemented')
        if int(start_step) < 0:
            raise ValueError('start_step must be >= 0')
        eps = opt_eps(optimizer, eps)
        self.lib = _lib.load()
        n_users, dim = user_emb.shape
        n_items = item_emb.shape[0]
        _chk(user_emb, torch.float32, 'user_emb')
        _chk(item_emb, torch.float32, 'item_emb', (n_items, dim))
        for t, name, n in ((item_bias, 'item_bias', n_items), (user_bias, 'user_bias', n_users),
                           (global_bias, 'global_bias', 1)):
            _chk(t, torch.float32, name, optional=True)
            if t is not None and t.numel() != n:
                raise ValueError(f'{name} has {t.numel()} elements, expected {n}')
        dev = user_emb.device
        self.device = dev
        self.params = dict(user_emb=user_emb, item_emb=item_emb, item_bias=item_bias, user_bias=user_bias,
                           global_bias=global_bias)
        self.m = {k: (torch.zeros_like(t) if t is not None else None) for k, t in self.params.items()}
        self.v = {k: (torch.zeros_like(t) if t is not None else None) for k, t in self.params.items()}
        self.loss_out = torch.zeros(2, dtype=torch.float64, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.max_batch, self.max_cols = int(max_batch), int(max_cols)
        nbytes = self.lib.hsk_bprmf_workspace_bytes(n_users, n_items, dim, self.max_batch, self.max_cols)
        if nbytes <= 0:
            raise ValueError('invalid workspace request')
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.csr_indptr, self.csr_indices, self.coo_user, self.coo_item = csr_indptr, csr_indices, coo_user, coo_item
        if csr_indptr is not None:
            _chk(csr_indptr, torch.int64, 'csr_indptr', (n_users + 1,))
            _chk(csr_indices, torch.int32, 'csr_indices')
            _chk(coo_user, torch.int32, 'coo_user')
            _chk(coo_item, torch.int32, 'coo_item', tuple(coo_user.shape))

        st = HskBprmfState()
        for k, t in self.params.items():
            setattr(st, k, _p(t))
            setattr(st, 'm_' + k, _p(self.m[k]))
            setattr(st, 'v_' + k, _p(self.v[k]))
        st.n_users, st.n_items, st.dim = n_users, n_items, dim
        st.lr, st.beta1, st.beta2, st.eps, st.wd = lr, beta1, beta2, eps, wd
        st.opt_kind = OPT_KINDS[optimizer]
        if lazy_items == 'auto':   # worth it when most item rows are outside every batch AND the dense sweep is not
            # small change anyway (a table of a few MB is swept in microseconds, inside the item pass's launch)
            lazy_items = (dim % 2 == 0 and n_items >= 2 * self.max_batch * self.max_cols
                          and n_items * dim > LAZY_USERS_MIN_ELEMENTS)
        st.lazy_items = 1 if lazy_items else 0
        st.step = int(start_step)   # hsk_bprmf_init_workspace stamps every row as current at this step
        st.csr_indptr, st.csr_indices = _p(csr_indptr), _p(csr_indices)
        st.coo_user, st.coo_item = _p(coo_user), _p(coo_item)
        st.nnz = 0 if coo_user is None else coo_user.numel()
        st.seed = seed & 0xFFFFFFFFFFFFFFFF
        st.workspace, st.workspace_bytes = _p(self.workspace), nbytes
        st.max_batch, st.max_cols = self.max_batch, self.max_cols
        # exact lazy AdamW on user rows (bit-identical to the dense sweep after flush()); dense when False.  'auto':
        # a table of only a few batches' worth of rows is swept densely inside the item pass's launch (measured at the
        # ml100k shape, U = 943, B = 128: 17.2 vs 19.4 us per step); beyond that only the batch's rows are touched
        # (ml1m shape, U = 6040: 31.6 vs 35.9 us)
        if lazy_users == 'auto':
            lazy_users = n_users > 8 * self.max_batch
        st.lazy_users = 1 if lazy_users else 0
        # steps_sampled() replays its steady-state loop as HIP graphs of this many steps (0: default 64, < 0: never)
        st.graph_chunk = int(graph_chunk)
        st.catchup_apart = 0
        # form of the large-batch item pass: 0 by the library's rule, 1 / -1 the pair form forced on / off (same bits)
        st.item_pair = 0
        # gather loop of the large-batch forward: 0 the library's choice, 1 / -1 the overlapped loop on / off (same bits)
        st.fwd_overlap = 0
        # the pair form's list weights / user rows: 0 the library's choice, 1 / -1 written in list order by a launch of
        # their own (k_item_lists) / gathered by every item wave (same bits)
        st.item_lists = 0
        # steps between the periodic sweeps of the lazily updated tables; 0: from the table / batch sizes
        # (hsk_bprmf_flush_cadence; a speed matter only -- every cadence gives the same bits)
        st.flush_every, st.ws_sharded = int(flush_every), 0
        st.timing_mask = 0
        if loss not in LOSS_KINDS:
            raise ValueError(f'unknown loss {loss!r}')
        if loss == 'bce' and (user_bias is not None or global_bias is not None):
            raise ValueError('the fused bce step treats user/global bias as gradient-free; use the autograd path')
        st.loss_kind, st.ssm_log_adjust = LOSS_KINDS[loss], float(log_adjust)
        self.alias = alias   # (prob f32 [I], idx i32 [I]) for train_neg_strategy 'popular', None = uniform
        if alias is not None:
            _chk(alias[0], torch.float32, 'alias prob', (n_items,))
            _chk(alias[1], torch.int32, 'alias idx', (n_items,))
        st.alias_prob, st.alias_idx = (None, None) if alias is None else (_p(alias[0]), _p(alias[1]))
        st.timing = None
        st.timing_every = 1
        self._timing = None
        # optional side stream: the batch named by hint_next() is sampled and item-sorted there while the current
        # step's item / user passes run (cross-step prefetch; results identical to the un-hinted sequence)
        self._aux = self.lib.hsk_aux_create() if overlap else None
        self._hint_order = None
        st.aux = self._aux
        st.loss_out, st.status = _p(self.loss_out), _p(self.status)
        self.st = st
        _lib.check(self.lib.hsk_bprmf_init_workspace(ctypes.byref(st), _stream()), 'hsk_bprmf_init_workspace')

    @property
    def step_count(self) -> int:
        return int(self.st.step)

    def step(self, u_idx: torch.Tensor, i_idx: torch.Tensor):
        """One fused step on a loader-provided batch (u_idx [B] int64, i_idx [B,1+N] int64)."""
        _chk(u_idx, torch.int64, 'u_idx')
        _chk(i_idx, torch.int64, 'i_idx')
        if i_idx.dim() != 2 or u_idx.shape != (i_idx.shape[0],):
            raise ValueError(f'u_idx {tuple(u_idx.shape)} / i_idx {tuple(i_idx.shape)}: expected [B] and [B,1+N]')
        B, K = i_idx.shape
        _lib.check(self.lib.hsk_bprmf_train_step(ctypes.byref(self.st), _p(u_idx), _p(i_idx), B, K, _stream()),
                   'hsk_bprmf_train_step')

    def step_sampled(self, order: Optional[torch.Tensor], start: int, batch: int, n_neg: int):
        """One fused step; positives = interactions order[start:start+batch], negatives drawn on device."""
        if order is not None:
            _chk(order, torch.int64, 'order')
            if start + batch > order.numel():
                raise ValueError('order too short')
        _lib.check(self.lib.hsk_bprmf_train_step_sampled(ctypes.byref(self.st), _p(order), start, batch, n_neg,
                                                         _stream()), 'hsk_bprmf_train_step_sampled')

    def steps_sampled(self, order: Optional[torch.Tensor], start: int, n_steps: int, batch: int, n_neg: int):
        """n_steps fused steps on consecutive batches of `batch` positives starting at order[start] -- the epoch's
        inner loop issued from C (each step hints the next one to the prefetch)."""
        if order is not None:
            _chk(order, torch.int64, 'order')
            if start + n_steps * batch > order.numel():
                raise ValueError('order too short')
        _lib.check(self.lib.hsk_bprmf_train_steps(ctypes.byref(self.st), _p(order), start, n_steps, batch, n_neg,
                                                  _stream()), 'hsk_bprmf_train_steps')

    def flush_cadence(self, batch: Optional[int] = None):
        """(steps between sweeps of the user table, of the item table) for batches of `batch` positives;
        2**30 = never (only flush() sweeps)."""
        import math
        b = self.max_batch if batch is None else int(batch)
        n_items = self.params['item_emb'].shape[0]
        touched = max(1, int(n_items * (1.0 - math.exp(-b * self.max_cols / n_items))))
        ref = ctypes.byref(self.st)
        return int(self.lib.hsk_bprmf_flush_cadence(ref, 0, b)), int(self.lib.hsk_bprmf_flush_cadence(ref, 1, touched))

    def graph_replays(self) -> int:
        """Runs of steps_sampled() issued as replayed HIP graphs so far."""
        return int(self.lib.hsk_bprmf_graph_replays(ctypes.byref(self.st)))

    def pipelined_steps(self) -> int:
        """Steps of steps_sampled() issued with the next batches' preparation riding in the steps' own launches."""
        return int(self.lib.hsk_bprmf_pipelined_steps(ctypes.byref(self.st)))

    def hint_next(self, order: Optional[torch.Tensor], start: int, batch: int, n_neg: int):
        """Name the batch of the NEXT step_sampled call so that the step issued now prepares it on the side stream.
        No-op without overlap=True.  batch <= 0 clears a pending hint."""
        if self._aux is None:
            return
        if order is not None and batch > 0:
            _chk(order, torch.int64, 'order')
            if start + batch > order.numel():
                raise ValueError('order too short')
        self._hint_order = order                      # keep the tensor alive until the hinted step was issued
        _lib.check(self.lib.hsk_bprmf_hint_next(ctypes.byref(self.st), _p(order), start, batch, n_neg),
                   'hsk_bprmf_hint_next')

    def hint_after_run(self, order: Optional[torch.Tensor], start: int, batch: int, n_neg: int, n_batches: int = 1):
        """Name the `n_batches` consecutive batches that follow the NEXT steps_sampled() run: the run's last steps prepare
        them (side stream, or -- large batches -- riding in the steps' own launches, which works two batches ahead), so
        an epoch issued in several runs keeps its preparation pipeline full.  No-op without overlap=True."""
        if self._aux is None:
            return
        self._hint_order = order
        _lib.check(self.lib.hsk_bprmf_hint_after_run_n(ctypes.byref(self.st), _p(order), start, batch, n_neg,
                                                       int(n_batches)), 'hsk_bprmf_hint_after_run_n')

    def last_batch(self, batch: int, n_cols: int):
        u = torch.empty(batch, dtype=torch.int64, device=self.device)
        i = torch.empty((batch, n_cols), dtype=torch.int64, device=self.device)
        _lib.check(self.lib.hsk_bprmf_last_batch(ctypes.byref(self.st), batch, n_cols, _p(u), _p(i), _stream()),
                   'hsk_bprmf_last_batch')
        return u, i

    def batch_columns(self, batch: int, n_cols: int) -> int:
        """Columns of the step's internal batch rows (n_cols, or n_cols + P - 1 under the item-partitioned forward)."""
        return int(self.lib.hsk_bprmf_batch_columns(ctypes.byref(self.st), batch, n_cols))

    def last_sort(self, n_entries: int):
        """(perm int32 [n_entries], offsets int32 [n_items + 1]): the item-major index of the last step's batch."""
        perm = torch.empty(n_entries, dtype=torch.int32, device=self.device)
        offs = torch.empty(self.params['item_emb'].shape[0] + 1, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.hsk_bprmf_last_sort(ctypes.byref(self.st), n_entries, _p(perm), _p(offs), _stream()),
                   'hsk_bprmf_last_sort')
        return perm, offs

    STAGES = ('prep', 'scan', 'scatter', 'fwd', 'item', 'user', 'finish')

    def enable_timing(self, stages=('fwd',), every=1):
        """Bracket the named stages of every `every`-th following step with HIP events on the launch stream."""
        if not getattr(self, '_timing', None):
            self._timing = self.lib.hsk_timing_create()
        mask = 0
        for s in stages:
            mask |= 1 << self.STAGES.index(s)
        self.st.timing = self._timing
        self.st.timing_mask = mask
        self.st.timing_every = int(every)

    def disable_timing(self):
        self.st.timing_mask = 0

    def collect_timing(self):
        """-> {stage: (total_ms, n_samples)}; waits for the recorded events."""
        if not getattr(self, '_timing', None):
            return {}
        n = len(self.STAGES)
        ms = (ctypes.c_double * n)()
        cnt = (ctypes.c_int64 * n)()
        _lib.check(self.lib.hsk_timing_collect(self._timing, ms, cnt), 'hsk_timing_collect')
        return {s: (ms[i], cnt[i]) for i, s in enumerate(self.STAGES) if cnt[i] > 0}

    def __del__(self):
        t = getattr(self, '_timing', None)
        if t:
            try:
                self.lib.hsk_timing_destroy(t)
            except Exception:
                pass
            self._timing = None
        a = getattr(self, '_aux', None)
        if a:
            try:
                torch.cuda.synchronize()
                self.lib.hsk_aux_destroy(a)
            except Exception:
                pass
            self._aux = None

    def flush(self):
        _lib.check(self.lib.hsk_bprmf_flush(ctypes.byref(self.st), _stream()), 'hsk_bprmf_flush')

    def set_hyper(self, lr=None, wd=None, beta1=None, beta2=None, eps=None):
        """Change the optimiser's hyper-parameters between steps (an LR schedule).  The library freezes them when the
        workspace is prepared -- the per-step Adam scalars of the lazy replay and of replayed graphs are a device table
        -- and refuses a step that finds them changed; this brings every row up to date under the OLD values (dense
        semantics: a pending zero-gradient step belongs to the schedule that was in force when it was due), installs the
        new ones and prepares the workspace again.  Loss sums and the step counter carry over."""
        self.flush()
        self.check_status()
        loss_sum = self.loss_out.clone()
        for name, val in (('lr', lr), ('wd', wd), ('beta1', beta1), ('beta2', beta2), ('eps', eps)):
            if val is not None:
                setattr(self.st, name, float(val))
        _lib.check(self.lib.hsk_bprmf_init_workspace(ctypes.byref(self.st), _stream()), 'hsk_bprmf_init_workspace')
        self.loss_out.copy_(loss_sum)

    def last_loss(self) -> float:
        return float(self.loss_out[0].item())

    def pop_loss_sum(self) -> float:
        """Sum of the per-step losses since the last call (one host sync)."""
        s = float(self.loss_out[1].item())
        self.loss_out[1].zero_()
        return s

    def check_status(self, what='fused BPR-MF step'):
        raise_on_status(self.status, what)


# ------------------------------------------------------------------------------------------------
# evaluation
# ------------------------------------------------------------------------------------------------
FUSED_TOPK_MAX_K = 128     # hsk_mf_eval_topk_fused (HSK_SEL_KMAX)
FUSED_TOPK_MIN_ITEMS = 20480   # below this many columns the materialised path is the faster one.  Round 4, with the in-GEMM
                               # selection on the 256 x 256 core, seeded and shared thresholds (csrc/hsk_eval_fused.hip:
                               # k_score_topk_wide): materialised / fused M users/s at U = 16 384 -- 16 384 items 6.85 / 6.15,
                               # 24 576: 3.88 / 4.38, 32 768: 2.98 / 3.57 (round 3's 128 x 128 selection crossed at 36 864)
_fused_ws = {}             # device -> scratch of the fused selection, grown on demand
_planes_ws = {}            # device -> scratch of the materialised path's operand pieces (fp16 pairs or bf16 triples), grown on demand


EVAL_ARITH_FP32, EVAL_ARITH_BF16X3, EVAL_ARITH_F16X2 = 0, 1, 2
EVAL_ARITH_DEFAULT = EVAL_ARITH_F16X2


def set_eval_arith(form=EVAL_ARITH_DEFAULT):
    """Arithmetic of the score GEMMs (materialised and fused top-k): 2 (default) two fp16 pieces per fp32 operand and three
    products on the 256 x 256 kernels (calls without the pieces' scratch or with rows that are not 16-byte aligned run
    form 1), 1 three bf16 pieces and six products, 0 exact fp32 MFMA; see hsk_eval_set_arith in include/hassaku_hip.h."""
    _lib.load().hsk_eval_set_arith(int(form))


def mf_eval_topk(user_emb, item_emb, item_bias, user_bias, global_bias, u_idx, k, excl_indptr=None, excl_indices=None,
                 item_begin=0, item_count=None, scores_ws=None, status=None, item_shard=False, n_items_global=None,
                 want_scores=None, presplit=True):
    """Top-k of one item shard's masked scores.  -> (vals [R,k] f32, idx [R,k] i32 global, scores or None).
    presplit=False withholds the scratch for the operands' pieces: the GEMM then cuts every tile into three bf16 pieces in
    its loop (form 1's bits whatever form is set; the form the library falls back to by itself, kept reachable for the
    parity test).
    want_scores=False: the selection runs inside the score GEMM and the score matrix is never formed (scores = None).
    want_scores=True (or a `scores_ws` buffer, k == 0, k > 128): the [R, item_count] matrix is materialised and
    returned.  None (default): whichever is faster for the shard width (FUSED_TOPK_MIN_ITEMS); same results.
    item_shard=True: `item_emb` / `item_bias` are the PHYSICAL shard (rows item_begin .. item_begin + item_count of a
    catalogue of n_items_global items); the library is handed the virtual base of the catalogue and only ever
    dereferences the shard's rows (include/hassaku_hip.h)."""
    _lib.require_gpu()
    lib = _lib.load()
    n_users, dim = user_emb.shape
    n_items = item_emb.shape[0]
    if item_shard:
        if item_count is None:
            item_count = n_items
        if item_count != n_items or n_items_global is None or item_begin + item_count > n_items_global:
            raise ValueError('item_shard: item_emb must hold exactly rows [item_begin, item_begin + item_count)')
    elif item_count is None:
        item_count = n_items - item_begin
    _chk(user_emb, torch.float32, 'user_emb')
    _chk(item_emb, torch.float32, 'item_emb', (n_items, dim))
    _chk(item_bias, torch.float32, 'item_bias', optional=True)
    if item_bias is not None and item_bias.numel() != n_items:
        raise ValueError('item_bias size mismatch')
    _chk(user_bias, torch.float32, 'user_bias', optional=True)
    _chk(global_bias, torch.float32, 'global_bias', optional=True)
    _chk(u_idx, torch.int64, 'u_idx')
    if excl_indptr is not None:
        _chk(excl_indptr, torch.int64, 'excl_indptr', (n_users + 1,))
        _chk(excl_indices, torch.int32, 'excl_indices')
    R = u_idx.numel()
    dev = user_emb.device
    if want_scores is None:
        want_scores = scores_ws is not None or item_count < FUSED_TOPK_MIN_ITEMS
    if not want_scores and scores_ws is None and 1 <= k <= FUSED_TOPK_MAX_K and R > 0:
        if presplit:
            need = lib.hsk_mf_eval_fused_ws_bytes_dim(R, item_count, k, dim)   # with room for the operands' pieces
        else:
            need = lib.hsk_mf_eval_fused_ws_bytes(R, item_count, k)
        if need <= 0:
            raise ValueError('invalid fused top-k request')
        ws = _fused_ws.get(dev)
        if ws is None or ws.numel() < need:
            ws = _fused_ws[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
        vals = torch.empty((R, k), dtype=torch.float32, device=dev)
        idx = torch.empty((R, k), dtype=torch.int32, device=dev)
        p_emb, p_bias, n_all = _p(item_emb), _p(item_bias), n_items
        if item_shard:
            p_emb -= 4 * dim * item_begin
            p_bias = None if p_bias is None else p_bias - 4 * item_begin
            n_all = n_items_global
        _lib.check(lib.hsk_mf_eval_topk_fused(_p(user_emb), p_emb, p_bias, _p(user_bias), _p(global_bias), n_users,
                                              n_all, dim, _p(u_idx), R, item_begin, item_count, _p(excl_indptr),
                                              _p(excl_indices), k, _p(ws), ws.numel() if presplit else need, _p(vals),
                                              _p(idx), _p(status),
                                              _stream()), 'hsk_mf_eval_topk_fused')
        return vals, idx, None
    if scores_ws is None:
        scores_ws = torch.empty((R, item_count), dtype=torch.float32, device=dev)
    else:
        _chk(scores_ws, torch.float32, 'scores_ws')
        if scores_ws.numel() < R * item_count:
            raise ValueError('scores_ws too small')
    vals = torch.empty((R, k), dtype=torch.float32, device=dev)
    idx = torch.empty((R, k), dtype=torch.int32, device=dev)
    p_emb, p_bias = _p(item_emb), _p(item_bias)
    if item_shard:
        p_emb -= 4 * dim * item_begin
        p_bias = None if p_bias is None else p_bias - 4 * item_begin
        n_items = n_items_global
    # scratch for the operands' pieces (split once per call instead of once per tile in the GEMM loop)
    need = lib.hsk_mf_eval_planes_bytes(R, item_count, dim)
    planes = _planes_ws.get(dev)
    if planes is None or planes.numel() < need:
        planes = _planes_ws[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
    _lib.check(lib.hsk_mf_eval_topk_planes(_p(user_emb), p_emb, p_bias, _p(user_bias), _p(global_bias),
                                           n_users, n_items, dim, _p(u_idx), R, item_begin, item_count,
                                           _p(excl_indptr), _p(excl_indices), k, _p(scores_ws),
                                           _p(planes) if presplit else None, planes.numel() if presplit else 0,
                                           _p(vals), _p(idx), _p(status), _stream()),
               'hsk_mf_eval_topk_planes')
    return vals, idx, scores_ws


def topk_dense(logits: torch.Tensor, k: int):
    """(values, indices int64) of the k largest entries per row; ties broken by lower index."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(logits, torch.float32, 'logits')
    if logits.dim() != 2:
        raise ValueError('logits must be 2-D')
    rows, cols = logits.shape
    vals = torch.empty((rows, k), dtype=torch.float32, device=logits.device)
    idx = torch.empty((rows, k), dtype=torch.int64, device=logits.device)
    _lib.check(lib.hsk_topk_dense(_p(logits), rows, cols, cols, k, _p(vals), _p(idx), _stream()), 'hsk_topk_dense')
    return vals, idx


def topk_merge(vals: torch.Tensor, idx: torch.Tensor):
    """[P,R,k] candidate lists -> global top-k [R,k]."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(vals, torch.float32, 'vals')
    _chk(idx, torch.int32, 'idx', tuple(vals.shape))
    P, R, k = vals.shape
    ov = torch.empty((R, k), dtype=torch.float32, device=vals.device)
    oi = torch.empty((R, k), dtype=torch.int32, device=vals.device)
    _lib.check(lib.hsk_topk_merge(_p(vals), _p(idx), P, R, k, _p(ov), _p(oi), _stream()), 'hsk_topk_merge')
    return ov, oi


def rank_metrics(topk_idx: torch.Tensor, u_idx: torch.Tensor, label_indptr: torch.Tensor,
                 label_indices: torch.Tensor, ks: Sequence[int]) -> torch.Tensor:
    """-> [R, len(ks), 3] (precision, recall, ndcg) per user and cut-off."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(topk_idx, torch.int32, 'topk_idx')
    _chk(u_idx, torch.int64, 'u_idx')
    _chk(label_indptr, torch.int64, 'label_indptr')
    _chk(label_indices, torch.int32, 'label_indices')
    R, kmax = topk_idx.shape
    if u_idx.shape != (R,):
        raise ValueError('u_idx / topk_idx row mismatch')
    ks_arr = (ctypes.c_int32 * len(ks))(*[int(x) for x in ks])
    out = torch.empty((R, len(ks), 3), dtype=torch.float32, device=topk_idx.device)
    _lib.check(lib.hsk_rank_metrics(_p(topk_idx), R, kmax, _p(u_idx), label_indptr.numel() - 1, _p(label_indptr),
                                    _p(label_indices), ks_arr,
                                    len(ks), _p(out), _stream()), 'hsk_rank_metrics')
    return out


def calibration_metrics(topk_idx: torch.Tensor, u_idx: torch.Tensor, item_mtx: torch.Tensor, user_mtx: torch.Tensor,
                        beta: float, ks: Sequence[int], status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> [R, len(ks), 3] fp64 (hellinger distance, jensen-shannon distance, kl divergence) per user and cut-off,
    between user_mtx[u] (fp64 [n_users, n_bins]) and the smoothed mean of the item_mtx rows (fp32 or fp64
    [n_items, n_bins], rows may be strided) of the first k ranked ids."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(topk_idx, torch.int32, 'topk_idx')
    _chk(u_idx, torch.int64, 'u_idx')
    _chk(user_mtx, torch.float64, 'user_mtx')
    _chk(status, torch.int32, 'status', (1,), optional=True)
    if item_mtx is None or not item_mtx.is_cuda:
        raise RuntimeError('item_mtx must live on the HIP device; there is no CPU path')
    if item_mtx.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'item_mtx must be float32 or float64, got {item_mtx.dtype}')
    if topk_idx.dim() != 2 or user_mtx.dim() != 2 or item_mtx.dim() != 2:
        raise ValueError('topk_idx, item_mtx and user_mtx must be 2-D')
    R, kmax = topk_idx.shape
    n_items, n_bins = item_mtx.shape
    if u_idx.shape != (R,):
        raise ValueError('u_idx / topk_idx row mismatch')
    if user_mtx.shape[1] != n_bins:
        raise ValueError(f'user_mtx has {user_mtx.shape[1]} bins, item_mtx {n_bins}')
    if item_mtx.stride(1) != 1 or item_mtx.stride(0) < n_bins:
        raise ValueError('item_mtx rows must be contiguous (a leading dimension >= n_bins is allowed)')
    ks_arr = (ctypes.c_int32 * len(ks))(*[int(x) for x in ks])
    out = torch.empty((R, len(ks), 3), dtype=torch.float64, device=topk_idx.device)
    _lib.check(lib.hsk_calibration_metrics(_p(topk_idx), R, kmax, _p(u_idx), _p(item_mtx),
                                           int(item_mtx.dtype == torch.float64), n_items, n_bins, item_mtx.stride(0),
                                           _p(user_mtx), user_mtx.shape[0], n_bins, float(beta), ks_arr, len(ks),
                                           _p(out), _p(status), _stream()), 'hsk_calibration_metrics')
    return out


# ---------------------------------------------------------------------------------------------------
# shared by the row scorers of the fitted models (knn, ease, p3, svd)
# ---------------------------------------------------------------------------------------------------
def _excl_pair(excl):
    """(indptr, indices) of an exclusion CSR, checked, or (None, None)."""
    if excl is None:
        return None, None
    ep, ei = excl
    _chk(ep, torch.int64, 'excl_indptr')
    _chk(ei, torch.int32, 'excl_indices')
    return ep, ei


def _score_out(out: Optional[torch.Tensor], R: int, n_cols: int, device) -> torch.Tensor:
    """The fp64 score buffer of R rows x n_cols columns: `out` checked, or a new one."""
    if out is None:
        out = torch.empty((R, n_cols), dtype=torch.float64, device=device)
    _chk(out, torch.float64, 'out')
    if out.dim() != 2 or out.shape[0] < R or out.shape[1] < n_cols:
        raise ValueError(f'out has shape {tuple(out.shape)}, needs at least ({R}, {n_cols})')
    return out


def _status_word(status: Optional[torch.Tensor], device) -> torch.Tensor:
    return torch.zeros(1, dtype=torch.int32, device=device) if status is None else status


# ---------------------------------------------------------------------------------------------------
# ItemKNN / UserKNN (hsk_knn.hip)
# ---------------------------------------------------------------------------------------------------
KNN_KINDS = {'cosine': 0, 'jaccard': 1, 'sorensen_dice': 2, 'asymmetric_cosine': 3, 'tversky': 4}
KNN_MAX_K = 1024
KNN_MAX_WINDOW = 20480


def knn_pack_dims(n_rows: int, n_cols: int) -> Tuple[int, int]:
    """(rows_pad, k_pad) of the int8 entity operand of an [n_rows, n_cols] binary matrix."""
    lib = _lib.load()
    rp, kp = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(lib.hsk_knn_pack_dims(int(n_rows), int(n_cols), ctypes.byref(rp), ctypes.byref(kp)), 'hsk_knn_pack_dims')
    return rp.value, kp.value


def knn_pack_i8(indptr: torch.Tensor, indices: torch.Tensor, n_rows: int, n_cols: int) -> torch.Tensor:
    """Binary CSR -> dense int8 [rows_pad, k_pad] (zero padded)."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(indptr, torch.int64, 'indptr', (n_rows + 1,))
    _chk(indices, torch.int32, 'indices')
    rp, kp = knn_pack_dims(n_rows, n_cols)
    out = torch.empty((rp, kp), dtype=torch.int8, device=indptr.device)
    _lib.check(lib.hsk_knn_pack_i8(_p(indptr), _p(indices), n_rows, n_cols, rp, kp, _p(out), _stream()),
               'hsk_knn_pack_i8')
    return out


def knn_gram_i8(M: torch.Tensor, n_rows: int, r0: int, r1: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 counts C[r - r0, c] = <M[r], M[c]> for r in [r0, r1), c < n_rows (r0 a multiple of 128)."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(M, torch.int8, 'M')
    rp, kp = M.shape
    if out is None:
        out = torch.empty((r1 - r0, n_rows), dtype=torch.int32, device=M.device)
    _chk(out, torch.int32, 'out')
    if out.dim() != 2 or out.shape[0] < r1 - r0 or out.shape[1] < n_rows:
        raise ValueError(f'out has shape {tuple(out.shape)}, needs at least ({r1 - r0}, {n_rows})')
    _lib.check(lib.hsk_knn_gram_i8(_p(M), n_rows, rp, kp, r0, r1, _p(out), out.shape[1], _stream()), 'hsk_knn_gram_i8')
    return out


def knn_select(C: torch.Tensor, rows: int, row0: int, deg: torch.Tensor, sqrt_deg: Optional[torch.Tensor],
               deg_alpha: Optional[torch.Tensor], deg_1m_alpha: Optional[torch.Tensor], kind: str, alpha: float,
               beta: float, shrinkage: float, k: int):
    """(idx int32 [rows, k], val fp64 [rows, k], len int32 [rows]) of the count block C (rows of C = entities row0...)."""
    _lib.require_gpu()
    lib = _lib.load()
    if kind not in KNN_KINDS:
        raise ValueError(f'unknown similarity {kind!r} (one of {sorted(KNN_KINDS)})')
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f'k = {k} outside [1, {KNN_MAX_K}]')
    _chk(C, torch.int32, 'C')
    n = deg.numel()
    _chk(deg, torch.int64, 'deg', (n,))
    for name, t in (('sqrt_deg', sqrt_deg), ('deg_alpha', deg_alpha), ('deg_1m_alpha', deg_1m_alpha)):
        _chk(t, torch.float64, name, (n,), optional=True)
    dev = C.device
    idx = torch.empty((rows, k), dtype=torch.int32, device=dev)
    val = torch.empty((rows, k), dtype=torch.float64, device=dev)
    ln = torch.empty(rows, dtype=torch.int32, device=dev)
    _lib.check(lib.hsk_knn_select(_p(C), rows, n, C.shape[1], row0, _p(deg), _p(sqrt_deg), _p(deg_alpha),
                                  _p(deg_1m_alpha), KNN_KINDS[kind], float(alpha or 0.), float(beta or 0.),
                                  float(shrinkage), k, _p(idx), _p(val), _p(ln), _stream()), 'hsk_knn_select')
    return idx, val, ln


def knn_score_rows(users: torch.Tensor, a_csr, b_csr, n_cols: int, window: int = 4096, excl=None,
                   out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp64 [R, n_cols]: row q = sum over A-row users[q] (stored order) of w_a * B-row.  a_csr / b_csr:
    (indptr int64, indices int32, vals fp64 or None, n_rows); excl: (indptr, indices) -> those columns -inf."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(users, torch.int64, 'users')
    R = users.numel()
    (ap, ai, av, an), (bp, bi, bv, bn) = a_csr, b_csr
    for name, (p, i, v, nr) in (('a', a_csr), ('b', b_csr)):
        _chk(p, torch.int64, f'{name}_indptr', (nr + 1,))
        _chk(i, torch.int32, f'{name}_indices')
        _chk(v, torch.float64, f'{name}_vals', (i.numel(),), optional=True)
    ep, ei = _excl_pair(excl)
    out, status = _score_out(out, R, n_cols, users.device), _status_word(status, users.device)
    window = max(1, min(int(window), KNN_MAX_WINDOW))
    _lib.check(lib.hsk_knn_score_rows(_p(users), R, an, _p(ap), _p(ai), _p(av), bn, _p(bp), _p(bi), _p(bv), n_cols,
                                      window, _p(ep), _p(ei), _p(out), out.shape[1], _p(status), _stream()),
               'hsk_knn_score_rows')
    return out


def knn_topk_rows(scores: torch.Tensor, k: int, n_cols: Optional[int] = None):
    """(values fp64 [R, k], ids int32 [R, k]) of each row's k largest, ties to the lower index."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(scores, torch.float64, 'scores')
    R, ld = scores.shape
    n_cols = ld if n_cols is None else n_cols
    vals = torch.empty((R, k), dtype=torch.float64, device=scores.device)
    ids = torch.empty((R, k), dtype=torch.int32, device=scores.device)
    _lib.check(lib.hsk_knn_topk_rows(_p(scores), R, n_cols, ld, k, _p(vals), _p(ids), _stream()), 'hsk_knn_topk_rows')
    return vals, ids


# ---------------------------------------------------------------------------------------------------
# EASE (hsk_ease.hip)
# ---------------------------------------------------------------------------------------------------
STATUS_NOT_SPD = 8


def ease_gram_f64(C: torch.Tensor, rows: int, r0: int, lam: int, G: torch.Tensor) -> torch.Tensor:
    """Rows [r0, r0 + rows) of the fp64 G = counts + lam I from an int32 count block of knn_gram_i8."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(C, torch.int32, 'C')
    n, _ = _chk_gram(G, 'G')
    if C.dim() != 2 or C.shape[0] < rows or C.shape[1] < n or r0 + rows > n:
        raise ValueError(f'G {tuple(G.shape)} / C {tuple(C.shape)} do not hold rows [{r0}, {r0 + rows}) of an n x n Gram')
    _lib.check(lib.hsk_ease_gram_f64(_p(C), rows, n, C.shape[1], r0, int(lam), _p(G), G.shape[1], _stream()),
               'hsk_ease_gram_f64')
    return G


def ease_inverse_ws_bytes(n: int) -> int:
    return int(_lib.load().hsk_ease_inverse_ws_bytes(int(n)))


def ease_inverse_f64(A: torch.Tensor, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In-place inverse of the SPD fp64 matrix A [n, ld >= n] (its first n columns).  Raises (after a synchronising
    read of the status word) if a pivot was not positive and finite."""
    _lib.require_gpu()
    lib = _lib.load()
    n, ld = _chk_gram(A, 'A')
    own = status is None
    if own:
        status = torch.zeros(1, dtype=torch.int32, device=A.device)
    ws = torch.empty(ease_inverse_ws_bytes(n) // 8, dtype=torch.float64, device=A.device)
    _lib.check(lib.hsk_ease_inverse_f64(_p(A), n, ld, _p(ws), ws.numel() * 8, _p(status), _stream()),
               'hsk_ease_inverse_f64')
    if own and int(status.item()) & STATUS_NOT_SPD:
        raise ArithmeticError('ease_inverse_f64: the matrix is not positive definite in fp64 (bad pivot)')
    return A


def ease_weights(P: torch.Tensor) -> torch.Tensor:
    """In place B = P / (-diag P) with a zero diagonal."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk_gram(P, 'P')
    nd = torch.empty(P.shape[0], dtype=torch.float64, device=P.device)
    _lib.check(lib.hsk_ease_weights(_p(P), P.shape[0], P.shape[1], _p(nd), _stream()), 'hsk_ease_weights')
    return P


def _gather_score_rows(users, x_csr, W, name, scale, window, excl, out, status):
    """ease_score_rows (scale None) and p3_score_rows (scale = (inv_deg_u, alpha)): hsk_gather_score.h's two entry
    points."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(users, torch.int64, 'users')
    R = users.numel()
    xp, xi, n_users = x_csr
    _chk(xp, torch.int64, 'x_indptr', (n_users + 1,))
    _chk(xi, torch.int32, 'x_indices')
    n_items, _ = _chk_gram(W, name)
    if scale is not None:
        inv_deg_u, alpha = scale
        if inv_deg_u.numel() < n_users:
            raise ValueError(f'inv_deg_u has {inv_deg_u.numel()} entries, needs {n_users}')
        _chk(inv_deg_u, torch.float64, 'inv_deg_u')
    ep, ei = _excl_pair(excl)
    out, status = _score_out(out, R, n_items, users.device), _status_word(status, users.device)
    head = (_p(users), R, n_users, _p(xp), _p(xi), _p(W), n_items, W.shape[1])
    tail = (max(1, int(window)), _p(ep), _p(ei), _p(out), out.shape[1], _p(status), _stream())
    if scale is None:
        _lib.check(lib.hsk_ease_score_rows(*head, *tail), 'hsk_ease_score_rows')
    else:
        _lib.check(lib.hsk_p3_score_rows(*head, _p(inv_deg_u), float(alpha), *tail), 'hsk_p3_score_rows')
    return out


def ease_score_rows(users: torch.Tensor, x_csr, B: torch.Tensor, window: int = 1024, excl=None,
                    out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp64 [R, n_items]: row q = sum of the rows of B picked by the items of train row users[q], in stored order.
    x_csr: (indptr int64, indices int32, n_users); excl: (indptr, indices) -> those columns -inf."""
    return _gather_score_rows(users, x_csr, B, 'B', None, window, excl, out, status)


# ---------------------------------------------------------------------------------------------------
# P3alpha (hsk_p3.hip)
# ---------------------------------------------------------------------------------------------------
def p3_inv_degrees(indptr: torch.Tensor, n_out: Optional[int] = None) -> torch.Tensor:
    """fp64 [n_out >= n]: 1 / degree of each row of a CSR (indptr int64 [n + 1]), 0.0 for degree 0 and for padding."""
    _lib.require_gpu()
    lib = _lib.load()
    n = indptr.numel() - 1
    _chk(indptr, torch.int64, 'indptr', (n + 1,))
    n_out = n if n_out is None else int(n_out)
    out = torch.empty(n_out, dtype=torch.float64, device=indptr.device)
    _lib.check(lib.hsk_p3_inv_degrees(_p(indptr), n, _p(out), n_out, _stream()), 'hsk_p3_inv_degrees')
    return out


def p3_gram_f64(M: torch.Tensor, n: int, col_weight: torch.Tensor, r0: int, r1: int, out: torch.Tensor,
                row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Rows [r0, r1) of out[i, j] = row_scale[i] * sum_u M[i, u] col_weight[u] M[j, u] (fp64 matrix cores) from the
    int8 image M [rows_pad, k_pad] of knn_pack_i8; col_weight fp64 [k_pad]; out fp64 [n, ld >= n]; r0 a multiple of
    128."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(M, torch.int8, 'M')
    rp, kp = M.shape
    _chk(col_weight, torch.float64, 'col_weight', (kp,))
    _chk(row_scale, torch.float64, 'row_scale', (n,), optional=True)
    _chk(out, torch.float64, 'out')
    if out.dim() != 2 or out.shape[0] < n or out.shape[1] < n:
        raise ValueError(f'out has shape {tuple(out.shape)}, needs at least ({n}, {n})')
    _lib.check(lib.hsk_p3_gram_f64(_p(M), n, rp, kp, _p(col_weight), _p(row_scale), r0, r1, _p(out), out.shape[1],
                                   _stream()), 'hsk_p3_gram_f64')
    return out


def p3_score_rows(users: torch.Tensor, x_csr, W: torch.Tensor, inv_deg_u: torch.Tensor, alpha: float,
                  window: int = 1024, excl=None, out: Optional[torch.Tensor] = None,
                  status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp64 [R, n_items]: row q = (inv_deg_u[u] * sum of the rows of W picked by the items of train row u = users[q],
    in stored order) ** alpha.  x_csr: (indptr int64, indices int32, n_users); excl: (indptr, indices) -> those
    columns -inf."""
    return _gather_score_rows(users, x_csr, W, 'W', (inv_deg_u, alpha), window, excl, out, status)


# ---------------------------------------------------------------------------------------------------
# SVD (hsk_svd.hip)
# ---------------------------------------------------------------------------------------------------
SVD_MAX_BLOCK = 512    # HSK_SVD_MAX_BLOCK: a wider block is refused by the library (error code), not here


def svd_ld(b: int) -> int:
    """The leading dimension of a freshly allocated block of width b: b rounded up to even."""
    return int(b) + (int(b) & 1)


def svd_empty(n: int, b: int, device) -> torch.Tensor:
    """An uninitialised fp64 [n, b] block whose rows are 16-byte aligned (a view of an [n, svd_ld(b)] buffer)."""
    return torch.empty((n, svd_ld(b)), dtype=torch.float64, device=device)[:, :b]


def _svd_dense(t: torch.Tensor, name: str, even: bool = True):
    """(rows, width, ld) of a row-major fp64 block: a 2-D tensor, or a column slice [:, :b] of one, on the device,
    16-byte aligned, with unit column stride and (if `even`) an even row stride >= its width."""
    if t is None:
        raise ValueError(f'{name} must not be None')
    if not t.is_cuda:
        raise RuntimeError(f'{name} must live on the HIP device (got {t.device}); there is no CPU path')
    if t.dtype != torch.float64:
        raise TypeError(f'{name} must be torch.float64, got {t.dtype}')
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f'{name} has shape {tuple(t.shape)}, expected a non-empty 2-D block')
    rows, width = t.shape
    ld = t.stride(0) if rows > 1 else max(t.stride(0), svd_ld(width) if even else width)
    if t.stride(1) != 1 or ld < width or (even and ld % 2):
        raise ValueError(f'{name} (strides {t.stride()}) must be row-major with a'
                         f'{"n even" if even else ""} leading dimension >= {width}')
    if even and t.data_ptr() % 16:
        raise ValueError(f'{name} must be 16-byte aligned')
    return rows, width, ld


def svd_spmm(csr, V: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp64 [n_rows, b]: CSR @ V with every stored entry 1, each sum in stored order from 0.0 (bitwise scipy's
    csr @ dense).  csr: (indptr int64 [n_rows + 1], indices int32, n_cols); V [n_cols, b]."""
    _lib.require_gpu()
    lib = _lib.load()
    ptr, idx, n_cols = csr
    n_rows = ptr.numel() - 1
    _chk(ptr, torch.int64, 'indptr', (n_rows + 1,))
    _chk(idx, torch.int32, 'indices')
    vr, b, ldv = _svd_dense(V, 'V')
    if vr != n_cols or n_rows < 1:
        raise ValueError(f'V has {vr} rows, the CSR {n_cols} columns and {n_rows} rows')
    if out is None:
        out = svd_empty(n_rows, b, V.device)
    orr, ob, ldo = _svd_dense(out, 'out')
    if (orr, ob) != (n_rows, b):
        raise ValueError(f'out has shape {tuple(out.shape)}, expected ({n_rows}, {b})')
    _lib.check(lib.hsk_svd_spmm_f64(_p(ptr), _p(idx), n_rows, n_cols, _p(V), ldv, b, _p(out), ldo, _stream()),
               'hsk_svd_spmm_f64')
    return out


def svd_gram_ws_bytes(n: int, b: int) -> int:
    return int(_lib.load().hsk_svd_gram_ws_bytes(int(n), int(b)))


def svd_gram(A: torch.Tensor, B: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp64 [b, b]: A^T B (B = A if not given) of two [n, b] blocks on the fp64 matrix cores; bitwise equal from call
    to call.  ws: a contiguous fp64 workspace of at least svd_gram_ws_bytes(n, b) bytes (allocated if not given);
    out: a contiguous fp64 [b, b] tensor to write (allocated if not given)."""
    _lib.require_gpu()
    lib = _lib.load()
    B = A if B is None else B
    n, b, lda = _svd_dense(A, 'A')
    nb, bb, ldb = _svd_dense(B, 'B')
    if (nb, bb) != (n, b):
        raise ValueError(f'A {tuple(A.shape)} and B {tuple(B.shape)} differ in shape')
    need = svd_gram_ws_bytes(n, b)
    if ws is None:
        ws = torch.empty(max(need // 8, 2), dtype=torch.float64, device=A.device)
    _chk(ws, torch.float64, 'ws')
    if ws.numel() * 8 < need or ws.data_ptr() % 16:
        raise ValueError(f'ws holds {ws.numel() * 8} bytes, svd_gram needs {need}, 16-byte aligned')
    H = torch.empty((b, b), dtype=torch.float64, device=A.device) if out is None else out
    _chk(H, torch.float64, 'out', (b, b))
    _lib.check(lib.hsk_svd_gram_f64(_p(A), lda, _p(B), ldb, n, b, _p(H), b, _p(ws), ws.numel() * 8, _stream()),
               'hsk_svd_gram_f64')
    return H


def svd_mul(A: torch.Tensor, Q: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp64 [n, b2]: A Q with A [n, b], Q [b, b2], b2 <= b, on the fp64 matrix cores; out must not be A."""
    _lib.require_gpu()
    lib = _lib.load()
    n, b, lda = _svd_dense(A, 'A')
    qr, b2, ldq = _svd_dense(Q, 'Q')
    if qr != b or b2 > b:
        raise ValueError(f'Q has shape {tuple(Q.shape)}, expected ({b}, b2 <= {b})')
    if out is None:
        out = svd_empty(n, b2, A.device)
    orr, ob, ldo = _svd_dense(out, 'out', even=False)
    if (orr, ob) != (n, b2):
        raise ValueError(f'out has shape {tuple(out.shape)}, expected ({n}, {b2})')
    if out.data_ptr() == A.data_ptr():
        raise ValueError('svd_mul is not in place: out must not be A')
    _lib.check(lib.hsk_svd_mul_f64(_p(A), lda, n, b, _p(Q), ldq, b2, _p(out), ldo, _stream()), 'hsk_svd_mul_f64')
    return out


def svd_residuals(Y: torch.Tensor, V: torch.Tensor, theta: torch.Tensor) -> torch.Tensor:
    """fp64 [b]: || Y[:, j] - theta[j] V[:, j] ||_2 of two [n, b] blocks (theta = 0: the column norms of Y)."""
    _lib.require_gpu()
    lib = _lib.load()
    n, b, ldy = _svd_dense(Y, 'Y')
    nv, bv, ldv = _svd_dense(V, 'V')
    if (nv, bv) != (n, b):
        raise ValueError(f'Y {tuple(Y.shape)} and V {tuple(V.shape)} differ in shape')
    _chk(theta, torch.float64, 'theta', (b,))
    res = torch.empty(b, dtype=torch.float64, device=Y.device)
    _lib.check(lib.hsk_svd_residuals_f64(_p(Y), ldy, _p(V), ldv, _p(theta), n, b, _p(res), _stream()),
               'hsk_svd_residuals_f64')
    return res


def svd_score_rows(users: torch.Tensor, UF: torch.Tensor, IF: torch.Tensor, excl=None,
                   out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp64 [R, n_items]: row q = UF[users[q]] @ IF^T (UF [n_users, k], IF [n_items, k]) on the fp64 matrix cores;
    excl: (indptr, indices) -> those columns -inf."""
    _lib.require_gpu()
    lib = _lib.load()
    _chk(users, torch.int64, 'users')
    R = users.numel()
    n_users, k, ldu = _svd_dense(UF, 'UF')
    n_items, ki, ldi = _svd_dense(IF, 'IF')
    if ki != k:
        raise ValueError(f'UF {tuple(UF.shape)} and IF {tuple(IF.shape)} differ in the number of factors')
    ep, ei = _excl_pair(excl)
    out, status = _score_out(out, R, n_items, users.device), _status_word(status, users.device)
    _lib.check(lib.hsk_svd_score_rows(_p(users), R, n_users, _p(UF), ldu, _p(IF), ldi, n_items, k, _p(ep), _p(ei),
                                      _p(out), out.shape[1], _p(status), _stream()), 'hsk_svd_score_rows')
    return out


# ---------------------------------------------------------------------------------------------------
# ALS (hsk_als.hip)
# ---------------------------------------------------------------------------------------------------
ALS_MAX_FACTORS = 128    # HSK_ALS_MAX_FACTORS: more factors are refused by the library (error code), not here


def als_solve(csr, Y: torch.Tensor, G: torch.Tensor, alpha: float, reg: float, order: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp64 [n_rows, k]: one ALS half-sweep, row r = (G + reg I + (alpha - 1) sum y_i y_i^T)^-1 (alpha sum y_i) over
    the column ids i of row r of the binary CSR, by Cholesky; a row without entries is exactly 0.  csr: (indptr int64
    [n_rows + 1], indices int32, n_cols); Y [n_cols, k] the other side's factors, G [k, k] = Y^T Y (svd_gram); order:
    int32 [n_rows], a permutation of the rows (the issue order; it changes no result).  status collects
    HSK_STATUS_BAD_INDEX (1: a column id out of range, skipped) and HSK_STATUS_NOT_SPD (8: the row is zeros)."""
    _lib.require_gpu()
    lib = _lib.load()
    ptr, idx, n_cols = csr
    n_rows = ptr.numel() - 1
    _chk(ptr, torch.int64, 'indptr', (n_rows + 1,))
    _chk(idx, torch.int32, 'indices')
    yr, k, ldy = _svd_dense(Y, 'Y')
    gr, gk, ldg = _svd_dense(G, 'G', even=False)
    if yr != n_cols or n_rows < 1:
        raise ValueError(f'Y has {yr} rows, the CSR {n_cols} columns and {n_rows} rows')
    if (gr, gk) != (k, k):
        raise ValueError(f'G has shape {tuple(G.shape)}, expected ({k}, {k})')
    _chk(order, torch.int32, 'order', (n_rows,), optional=True)
    if out is None:
        out = svd_empty(n_rows, k, Y.device)
    orr, ob, ldo = _svd_dense(out, 'out')
    if (orr, ob) != (n_rows, k):
        raise ValueError(f'out has shape {tuple(out.shape)}, expected ({n_rows}, {k})')
    status = _status_word(status, Y.device)
    _chk(status, torch.int32, 'status', (1,))
    _lib.check(lib.hsk_als_solve_f64(_p(ptr), _p(idx), n_rows, n_cols, _p(order), _p(Y), ldy, k, _p(G), ldg,
                                     float(alpha), float(reg), _p(out), ldo, _p(status), _stream()),
               'hsk_als_solve_f64')
    return out


# ---------------------------------------------------------------------------------------------------
# SLIM (hsk_slim.hip)
# ---------------------------------------------------------------------------------------------------
STATUS_NOT_FINITE = 16
SLIM_LDS_CANDIDATES = 4096   # SLIM_LDS_CANDIDATES of csrc/hsk_slim.hip: columns with more candidates use the workspace


def slim_ws_bytes(n: int) -> int:
    return int(_lib.load().hsk_slim_cd_ws_bytes(int(n)))


def slim_cd(G: torch.Tensor, l1: float, l2: float, tol: float, max_iter: int, j0: int = 0, j1: Optional[int] = None,
            out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None,
            status: Optional[torch.Tensor] = None):
    """(Wt fp64 [n, ld], n_iter int32 [n], gap fp64 [n]): cyclic coordinate descent of the SLIM columns [j0, j1) over
    the symmetric fp64 Gram G [n, ld >= n]; row j of Wt holds the non-negative weights of target item j (Wt[j, j] = 0),
    n_iter[j] the sweeps run and gap[j] the last duality gap.  Rows outside the range keep what `out` held (a new `out`
    is zeros); n_iter and gap are 0 there.  l1 = n_users alpha l1_ratio, l2 = n_users alpha (1 - l1_ratio); tol = 0
    runs max_iter sweeps unless a sweep changes nothing.  ws: a uint8 buffer of slim_ws_bytes(n).  status collects
    HSK_STATUS_NOT_FINITE (16); without a caller's word a set bit raises ArithmeticError here."""
    _lib.require_gpu()
    lib = _lib.load()
    n, ld = _chk_gram(G, 'G')
    j1 = n if j1 is None else j1
    if out is None:
        out = torch.zeros((n, n), dtype=torch.float64, device=G.device)
    _chk(out, torch.float64, 'out')
    if out.dim() != 2 or out.shape[0] != n or out.shape[1] < n:
        raise ValueError(f'out has shape {tuple(out.shape)}, expected [{n}, ld >= {n}]')
    need = slim_ws_bytes(n)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=G.device)
    _chk(ws, torch.uint8, 'ws')
    own = status is None
    status = _status_word(status, G.device)
    _chk(status, torch.int32, 'status', (1,))
    n_iter = torch.zeros(n, dtype=torch.int32, device=G.device)
    gap = torch.zeros(n, dtype=torch.float64, device=G.device)
    _lib.check(lib.hsk_slim_cd_f64(_p(G), n, ld, int(j0), int(j1), float(l1), float(l2), float(tol), int(max_iter),
                                   _p(out), out.shape[1], _p(n_iter), _p(gap), _p(ws), ws.numel(), _p(status),
                                   _stream()), 'hsk_slim_cd_f64')
    if own and int(status.item()) & STATUS_NOT_FINITE:
        raise ArithmeticError('slim_cd: a non-finite entry of G, weight or gap (HSK_STATUS_NOT_FINITE)')
    return out, n_iter, gap
