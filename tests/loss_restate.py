"""Plain float64 numpy restatement of one training step's loss and gradients for the three recommendation losses
(the reference's train/rec_losses.py:27-53 bce, :56-88 bpr, :91-139 sampled softmax), and the "dial tables" whose
scores are exact in fp32.  No kernel, no oracle: what tests/test_loss_range.py holds the HIP forwards to.

The score of entry (b, k) is  s = <user_emb[u_b], item_emb[i_bk]> + item_bias[i_bk].

  bpr              mean over (b, n >= 1) of softplus(-(s_b0 - s_bn))
  bce              mean over (b, k) of BCEWithLogits(s_bk, [k == 0])
  sampled_softmax  mean over b of -s_b0 + logsumexp(s_b0, s_b1 + c, ..., s_bN + c),  c = log_adjust

Everything is evaluated in forms that do not cancel (sigmoid through logaddexp, the positive's softmax weight minus one
as minus the sum of the others), so the float64 figures are good to ~1e-15 of each entry whatever the score range.

Dense gradients go through one scipy sparse [users x items] matrix W of the entry weights d loss / d s:
  d user_emb = W @ item_emb,  d item_emb = W.T @ user_emb,  d item_bias = column sums of W;
the same three products with |W| and |tables| give every gradient element its own scale  sum_k |g_k| |operand_k|.
"""
import numpy as np
import scipy.sparse as sp

LOSSES = ('bpr', 'bce', 'sampled_softmax')


# ------------------------------------------------------------------------------------------------
# dial tables
# ------------------------------------------------------------------------------------------------
DIAL_SPIKE = 104.0                   # the loudest dial; 'wide' dials stay within +-DIAL_WIDE so that a spike / floor item
DIAL_WIDE, DIAL_MID, DIAL_QUIET = 100.0, 12.0, 2.0   # is above / below every other item for every user
CLASSES = ('quiet', 'mid', 'wide', 'spike', 'floor')
CLASS_SHARE = (0.40, 0.20, 0.36, 0.02, 0.02)


def _sixteenths(rng, size, bound):
    """multiples of 1/16, uniform in [-bound, bound]"""
    n = int(round(bound * 16))
    return rng.randint(-n, n + 1, size=size) / 16.0


def dial_tables(rng, n_users, n_items, dim, dial_max=None):
    """-> (params {user_emb, item_emb, item_bias} float32, item class index [I] into CLASSES).

    Coordinates 0 .. D-2 are noise: nonzero with probability 1/8, value k/16 with k in [-8, 8].  Coordinate D-1 is the
    dial: 1.0 in every user row, dial[i] (a multiple of 1/16 in [-104, 104]) in item row i; item_bias holds multiples
    of 1/256 in [-0.25, 0.25].  Every product is a multiple of 2^-8 and every partial sum stays below 2^9, so a score is
    exact in fp32 in any summation order, with or without FMA.  An item's class says which range its dial was drawn
    from; `dial_max` caps all of them (the sharded test keeps the dials within +-40)."""
    def noise(rows):
        val = rng.randint(-8, 9, size=(rows, dim)) / 16.0
        return np.where(rng.randint(0, 8, size=(rows, dim)) == 0, val, 0.0)

    ue, ie = noise(n_users), noise(n_items)
    cls = rng.choice(len(CLASSES), size=n_items, p=CLASS_SHARE)
    cls[rng.permutation(n_items)[:len(CLASSES) * 4]] = np.repeat(np.arange(len(CLASSES)), 4)   # no class is empty
    dial = np.select([cls == 0, cls == 1, cls == 2, cls == 3],
                     [_sixteenths(rng, n_items, DIAL_QUIET), _sixteenths(rng, n_items, DIAL_MID),
                      _sixteenths(rng, n_items, DIAL_WIDE), np.full(n_items, DIAL_SPIKE)], -DIAL_SPIKE)
    if dial_max is not None:
        dial = np.where(np.abs(dial) > dial_max, _sixteenths(rng, n_items, dial_max), dial)
    ue[:, dim - 1] = 1.0
    ie[:, dim - 1] = dial
    ib = rng.randint(-64, 65, size=n_items) / 256.0
    P = {'user_emb': ue.astype(np.float32), 'item_emb': ie.astype(np.float32), 'item_bias': ib.astype(np.float32)}
    for k, a in (('user_emb', ue), ('item_emb', ie), ('item_bias', ib)):
        assert np.array_equal(P[k].astype(np.float64), a), k
    return P, cls


def init_tables(rng, n_users, n_items, dim):
    """the initialisation-scale tables every other training test uses"""
    return {'user_emb': (rng.randn(n_users, dim) * 0.05).astype(np.float32),
            'item_emb': (rng.randn(n_items, dim) * 0.05).astype(np.float32),
            'item_bias': (rng.randn(n_items) * 0.1).astype(np.float32)}


def score_matrix(P):
    """float64 [users, items]: user_emb @ item_emb.T + item_bias"""
    return P['user_emb'].astype(np.float64) @ P['item_emb'].astype(np.float64).T + P['item_bias'].astype(np.float64)


def batch_scores(P, u, i, S=None):
    """float64 [B, K] scores of a batch: the full product, then indexed (no [B, K, D] gather)"""
    S = score_matrix(P) if S is None else S
    return S[np.asarray(u)[:, None], np.asarray(i)]


# ------------------------------------------------------------------------------------------------
# losses on scores
# ------------------------------------------------------------------------------------------------
def _softplus(z):
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def _sigmoid(z):
    return np.exp(-np.logaddexp(0.0, -z))


def loss_and_entry_grads(s, loss, log_adjust=0.0):
    """s float64 [B, K] -> (loss, g = d loss / d s [B, K], aux).  aux['p'] (sampled softmax): the softmax weights."""
    s = np.asarray(s, dtype=np.float64)
    B, K = s.shape
    g = np.empty_like(s)
    aux = {}
    if loss == 'bpr':
        inv = 1.0 / (B * (K - 1))
        x = s[:, :1] - s[:, 1:]
        val = _softplus(-x).sum() * inv
        g[:, 1:] = _sigmoid(-x) * inv
        g[:, 0] = -g[:, 1:].sum(axis=1)
    elif loss == 'bce':
        inv = 1.0 / (B * K)
        val = (_softplus(-s[:, 0]).sum() + _softplus(s[:, 1:]).sum()) * inv
        g[:, 1:] = _sigmoid(s[:, 1:]) * inv
        g[:, 0] = -_sigmoid(-s[:, 0]) * inv
    elif loss == 'sampled_softmax':
        inv = 1.0 / B
        z = s.copy()
        z[:, 1:] += log_adjust
        mx = z.max(axis=1, keepdims=True)
        e = np.exp(z - mx)
        tot = e.sum(axis=1, keepdims=True)
        val = (-s[:, 0] + mx[:, 0] + np.log(tot[:, 0])).sum() * inv
        p = e / tot
        g[:, 1:] = p[:, 1:] * inv
        g[:, 0] = -(e[:, 1:].sum(axis=1) / tot[:, 0]) * inv     # p_0 - 1 without the cancellation
        aux['p'], aux['z'] = p, z
    else:
        raise ValueError(loss)
    return float(val), g, aux


# ------------------------------------------------------------------------------------------------
# dense gradients
# ------------------------------------------------------------------------------------------------
def dense_products(Ue, Ie, u, i, w):
    """Entry weights w [B, K] -> (W @ Ie [U, D], W.T @ Ue [I, D], column sums of W [I]),
    W the sparse [users x items] matrix that sums w over the entries of a (user, item) pair."""
    u, i = np.asarray(u, dtype=np.int64), np.asarray(i, dtype=np.int64)
    B, K = i.shape
    W = sp.coo_matrix((np.asarray(w, dtype=np.float64).reshape(-1), (np.repeat(u, K), i.reshape(-1))),
                      shape=(Ue.shape[0], Ie.shape[0])).tocsr()
    return W @ Ie, W.T.tocsr() @ Ue, np.asarray(W.sum(axis=0)).reshape(-1)


def restate(P, u, i, loss, log_adjust=0.0, S=None, scores=None):
    """One step's float64 figures.  P: {user_emb, item_emb, item_bias}; u [B]; i [B, 1 + N].

    -> dict: scores [B, K], loss, g [B, K] (d loss / d score), aux, grads {name: dense d loss / d table},
       scale {name: sum_k |g_k| |operand_k| per element}.
    `S` is a precomputed score_matrix(P); `scores` overrides the scores (a caller that wants the loss arithmetic of
    scores it rounded itself)."""
    Ue, Ie = P['user_emb'].astype(np.float64), P['item_emb'].astype(np.float64)
    s = batch_scores(P, u, i, S) if scores is None else np.asarray(scores, dtype=np.float64)
    val, g, aux = loss_and_entry_grads(s, loss, log_adjust)
    names = ('user_emb', 'item_emb', 'item_bias')
    return {'scores': s, 'loss': val, 'g': g, 'aux': aux,
            'grads': dict(zip(names, dense_products(Ue, Ie, u, i, g))),
            'scale': dict(zip(names, dense_products(np.abs(Ue), np.abs(Ie), u, i, np.abs(g))))}
