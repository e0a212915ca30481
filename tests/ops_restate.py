"""Plain float64 numpy restatement of the un-fused operators (hsk_mf_scores, hsk_mf_backward, hsk_embedding_gather and
their dim == 0 forms), written from the operators' contract (include/hassaku_hip.h, DESIGN sections 2 and 3) and not
from the kernels.  No kernel, no oracle, no torch: what tests/test_unfused_ops.py holds the HIP operators to.

  scores     s[b, k] = sum_d U[u_b, d] * I[i_bk, d]   then  + Ub[u_b],  + Ib[i_bk],  + gb   (absent biases are skipped;
             dim == 0: the tables are None and the score is the biases alone)
  backward   the dense gradients of  sum_bk g[b, k] * s[b, k]  with respect to U, I, Ib, Ub, gb, every occurrence of a row
             added (np.add.at), rows nobody indexed zero
  clamp      an index outside [0, n) reads row 0 (and raises the status bit, which is not restated here)
  tile       the row shape (V, NCH, FULL) a dimension is served with, None where it is refused

Every output element comes with its **scale**, the sum of the magnitudes of its terms, and its **term count** n, so a
caller can hold an fp32 result to a bound of its own: an integer-valued element whose scale is below 2^24 is exact in
fp32 whatever the order of its sum (every product and every partial sum is an integer below 2^24), a rounded one lies
within (roundings) * 2^-24 * scale of the float64 value.
"""
import numpy as np

EXACT_LIMIT = float(2 ** 24)     # integers up to here are fp32 numbers: sums whose scale stays below are order-free
U32 = 2.0 ** -24                 # unit roundoff of fp32
TINY, STEP = 2.0 ** -126, 2.0 ** -149   # below TINY an fp32 value is subnormal and moves in steps of STEP
WAVE_TREE = 6                    # stages of the sum over 64 lanes
BIAS_ADDS = 3


def clamp(idx, n):
    """The clamping rule: an index outside [0, n) reads row 0."""
    idx = np.asarray(idx, dtype=np.int64)
    return np.where((idx < 0) | (idx >= n), 0, idx)


def is_bad(idx, n):
    idx = np.asarray(idx, dtype=np.int64)
    return bool(((idx < 0) | (idx >= n)).any())


def tile(D):
    """(V, NCH, FULL) by the rule of DESIGN section 3, or None where the dimension is refused.  V floats per lane and
    chunk: 4 / 2 / 1 by the row's alignment; NCH chunks of 64 lanes: the power of two in 1 .. 8 that holds the row;
    FULL: a V = 4 row that fills every chunk (no tail predicate)."""
    D = int(D)
    if D < 1:
        return None
    V = 4 if D % 4 == 0 else 2 if D % 2 == 0 else 1
    chunks = -(-D // (64 * V))
    for nch in (1, 2, 4, 8):
        if chunks <= nch:
            return V, nch, V == 4 and D == 64 * V * nch
    return None


def max_dim(D):
    """The widest dimension of D's alignment that is served."""
    V = 4 if D % 4 == 0 else 2 if D % 2 == 0 else 1
    return 64 * V * 8


def score_rows_buffered(D):
    """R: item rows a wave of the score kernel keeps in flight (2 when a row takes 16 or more registers, else 4)."""
    V, NCH, _ = tile(D)
    return 2 if V * NCH >= 16 else 4


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def scores(U, I, Ib, Ub, gb, u, i):
    """-> (s, scale, n): float64 [B, K] scores, sum of |terms| per score, and the number of terms (D + biases present).
    U, I: [rows, D] or None (dim == 0); Ib [items], Ub [users], gb [1] or None; u [B], i [B, K] valid indices."""
    u, i = np.asarray(u, dtype=np.int64), np.asarray(i, dtype=np.int64)
    B, K = i.shape
    s, scale, n = np.zeros((B, K)), np.zeros((B, K)), 0
    if U is not None:
        U, I = _f64(U), _f64(I)
        if B * K * U.shape[1] <= 1 << 22:
            s = np.einsum('bd,bkd->bk', U[u], I[i])
            scale = np.einsum('bd,bkd->bk', np.abs(U[u]), np.abs(I[i]))
        else:
            for b in range(B):          # row by row: no large [B, K, D] gather
                rows = I[i[b]]
                s[b] = rows @ U[u[b]]
                scale[b] = np.abs(rows) @ np.abs(U[u[b]])
        n += U.shape[1]
    if Ub is not None:
        t = _f64(Ub).reshape(-1)[u][:, None]
        s, scale, n = s + t, scale + np.abs(t), n + 1
    if Ib is not None:
        t = _f64(Ib).reshape(-1)[i]
        s, scale, n = s + t, scale + np.abs(t), n + 1
    if gb is not None:
        t = float(_f64(gb).reshape(-1)[0])
        s, scale, n = s + t, scale + abs(t), n + 1
    return s, scale, n


def scores_bound(D, scale, ref):
    """The rounded scores' bound: the per-lane fmaf chain is NCH * V long, the wave tree has six stages, there are three
    bias adds; one 2^-24 of the score's scale each.  A subnormal score gets the same count of 2^-149 steps."""
    V, NCH, _ = tile(D) if D > 0 else (0, 0, False)
    c = NCH * V + WAVE_TREE + BIAS_ADDS
    tol = c * U32 * scale
    return np.where((np.abs(ref) < TINY) & (scale > 0), np.maximum(tol, c * STEP), tol)


def backward(U, I, u, i, g, n_users=None, n_items=None):
    """Dense gradients of sum(g * scores) -> {name: (grad, scale, n)} for name in user_emb, item_emb (absent when U is
    None), item_bias, user_bias, global_bias; grad and scale float64, n int64, all of the parameter's flat shape
    ([rows, D], [rows], [1]).  scale = sum of |g| * |operand| over the element's terms, n their number."""
    u, i, g = np.asarray(u, dtype=np.int64), np.asarray(i, dtype=np.int64), _f64(g)
    B, K = i.shape
    if U is not None:
        U, I = _f64(U), _f64(I)
        n_users, n_items = U.shape[0], I.shape[0]
    ag = np.abs(g)
    out = {}
    if U is not None:
        D = U.shape[1]
        gU, sU, gI, sI = np.zeros_like(U), np.zeros_like(U), np.zeros_like(I), np.zeros_like(I)
        aU, aI = np.abs(U), np.abs(I)
        for b in range(B):
            np.add.at(gU, u[b], g[b] @ I[i[b]])          # one user row: the K terms summed in float64, then added
            np.add.at(sU, u[b], ag[b] @ aI[i[b]])
            np.add.at(gI, i[b], g[b][:, None] * U[u[b]][None, :])
            np.add.at(sI, i[b], ag[b][:, None] * aU[u[b]][None, :])
        nU = np.zeros(n_users, dtype=np.int64)
        np.add.at(nU, u, K)
        nI = np.zeros(n_items, dtype=np.int64)
        np.add.at(nI, i.reshape(-1), 1)
        out['user_emb'] = (gU, sU, np.repeat(nU[:, None], D, axis=1))
        out['item_emb'] = (gI, sI, np.repeat(nI[:, None], D, axis=1))
    gIb, sIb, nIb = np.zeros(n_items), np.zeros(n_items), np.zeros(n_items, dtype=np.int64)
    np.add.at(gIb, i.reshape(-1), g.reshape(-1))
    np.add.at(sIb, i.reshape(-1), ag.reshape(-1))
    np.add.at(nIb, i.reshape(-1), 1)
    gUb, sUb, nUb = np.zeros(n_users), np.zeros(n_users), np.zeros(n_users, dtype=np.int64)
    np.add.at(gUb, u, g.sum(axis=1))
    np.add.at(sUb, u, ag.sum(axis=1))
    np.add.at(nUb, u, K)
    out['item_bias'] = (gIb, sIb, nIb)
    out['user_bias'] = (gUb, sUb, nUb)
    out['global_bias'] = (np.array([g.sum()]), np.array([ag.sum()]), np.array([B * K], dtype=np.int64))
    return out


def grad_bound(scale, n, ref):
    """The rounded gradients' bound: (n + 1) * 2^-24 * sum |terms| -- one rounding per product or addition of the
    element's n terms, in any order (so it covers the atomics); subnormal values the same count of 2^-149 steps."""
    tol = (n + 1) * U32 * scale
    return np.where((np.abs(ref) < TINY) & (scale > 0), np.maximum(tol, (n + 1) * STEP), tol)


def is_exact(scale):
    """The exactness precondition: every element's sum of |terms| is below 2^24."""
    return bool((np.asarray(scale) < EXACT_LIMIT).all())
