"""Restatements of ECF (Du et al., "Towards Explainable Collaborative Filtering with Taste Clusters Learning", WWW
2023) for the tests: written from the paper's formulas and the operator's definition in DESIGN 5.8, on dense matrices.

  affiliation / affiliation_backward   numpy, in the dtype asked for: float64 is the yardstick, float32 "the fp32 form"
  forward_f64                          the whole forward and the three losses in float64 torch (differentiable)
"""
import numpy as np
import torch


def topk_mask(S: np.ndarray, k: int) -> np.ndarray:
    """m[r, c] = 1 iff fewer than k entries j of row r have S[r, j] > S[r, c] or (S[r, j] == S[r, c] and j < c)."""
    bigger = S[:, None, :] > S[:, :, None]                         # [r, c, j]: S_j > S_c
    j_first = np.arange(S.shape[1])[None, :] < np.arange(S.shape[1])[:, None]      # [c, j]: j < c
    rank = (bigger | ((S[:, None, :] == S[:, :, None]) & j_first[None])).sum(-1)
    return rank < k


def _pieces(S, k, t, dtype):
    S = np.asarray(S, dtype)
    z = S / dtype(t)
    e = np.exp(z - z.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True, dtype=dtype)
    m = topk_mask(S, k).astype(dtype)
    mh = p + (m - p)
    # sigmoid and its derivative from e = exp(-|S|): sigmoid(|S|) = 1 / (1 + e), sigmoid(-|S|) = e / (1 + e),
    # sigmoid' = e / (1 + e)^2; accurate where the sigmoid saturates (1 - sigmoid would cancel to 0 there)
    e = np.exp(-np.abs(S))
    r = dtype(1) / (dtype(1) + e)
    return p, mh, np.where(S >= 0, r, e * r), e * r * r


def affiliation(S, k: int, t: float, dtype=np.float64) -> np.ndarray:
    _, mh, sig, _ = _pieces(S, k, t, dtype)
    return sig * mh


def affiliation_backward(S, G, k: int, t: float, dtype=np.float64) -> np.ndarray:
    p, mh, sig, dsig = _pieces(S, k, t, dtype)
    G = np.asarray(G, dtype)
    h = G * sig
    ph = (p * h).sum(-1, keepdims=True, dtype=dtype)
    return G * dsig * mh + (dtype(1) / dtype(t)) * (p * (h - ph))


# ------------------------------------------------------------------------------------------------ the model, float64
def _cosine(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    an = a / a.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    bn = b / b.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return (an @ bn.T).clamp(-1., 1.)


def _affiliate(S: torch.Tensor, k: int, t: float) -> torch.Tensor:
    """sigmoid(S) * (p + (m - p)) with the mask a constant: the gradient passes through p = softmax(S / t) only."""
    p = torch.softmax(S / t, dim=-1)
    m = torch.from_numpy(topk_mask(S.detach().numpy(), k)).to(S.dtype)
    return torch.sigmoid(S) * (p + (m - p).detach())


def forward_f64(user_embed, item_embed, clusters, X, T, u_idxs, i_idxs, top_n, top_m, temp_masking, temp_tags, top_p):
    """user_embed [U, D], item_embed [I, D], clusters [C, D]: float64 torch tensors (leaves that may require grad);
    X [U, I] the dense 0/1 train matrix, T [I, n_tags] the dense weighted tag matrix (float64 tensors); u_idxs [B],
    i_idxs [B, K] or [I'] (evaluation: a shared item list).  Returns a dict: x_tilde [I, C], xs [I, C], a [B, C],
    scores [B, K] / [B, I'], and the unweighted losses ts, ind, cf (cf only for the training shape)."""
    x_tilde = _cosine(item_embed, clusters)
    xs = _affiliate(x_tilde, top_m, temp_masking)
    a = _affiliate(X[u_idxs] @ x_tilde, top_n, temp_masking)
    x_i = xs[i_idxs]
    out = {'x_tilde': x_tilde, 'xs': xs, 'a': a}
    out['scores'] = a @ x_i.T if i_idxs.dim() == 1 else (a[:, None, :] * x_i).sum(-1)
    d_c = xs.T @ T                                                       # [C, n_tags]
    log_b = torch.log_softmax(d_c / temp_tags, dim=-1)
    out['log_b'] = log_b
    out['ts'] = -log_b.topk(top_p, dim=-1).values.sum()
    sim = _cosine(clusters, clusters)
    out['ind'] = -torch.log_softmax(sim, dim=-1).diagonal().sum()
    if i_idxs.dim() == 2:
        logits = (user_embed[u_idxs][:, None, :] * item_embed[i_idxs]).sum(-1)
        diff = (logits[:, :1] - logits[:, 1:]).flatten()
        out['cf'] = torch.nn.functional.softplus(-diff).mean()           # BCEWithLogits(diff, 1)
    return out


def bpr(scores: torch.Tensor) -> torch.Tensor:
    """The BPR loss on [B, 1 + neg] scores, positive first: the mean of -log sigmoid(pos - neg) over all B * neg pairs."""
    return torch.nn.functional.softplus(-(scores[:, :1] - scores[:, 1:])).mean()
