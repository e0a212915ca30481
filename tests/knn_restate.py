"""numpy-only float64 restatement of the reference's ItemKNN / UserKNN (utilities/similarities.py, knn_algs.py) --
the expected values of tests/test_knn.py.  tests/test_knn.py holds it to the g11 goldens bitwise on the CPU.

Ties are broken by the lower index (the build's rule; the reference's argsort / topk leave them arbitrary)."""
import numpy as np


def dense_binary(indptr, indices, n_rows, n_cols):
    M = np.zeros((n_rows, n_cols), np.float64)
    M[np.repeat(np.arange(n_rows), np.diff(indptr)), indices] = 1.
    return M


def similarity_rows(counts, rows, deg, sim, shrinkage, alpha=None, beta=None):
    """fp64 similarity of the count block `counts` [len(rows), n] (int64) in the reference's operation order."""
    c = counts.astype(np.float64)
    dr, dc = deg[rows][:, None], deg[None, :]
    with np.errstate(divide='ignore', invalid='ignore'):
        if sim == 'cosine':
            sq = np.sqrt(deg.astype(np.float64))
            v = c / (sq[rows][:, None] * sq[None, :])
        elif sim == 'jaccard':
            v = c / (dr + dc - counts).astype(np.float64)
        elif sim == 'sorensen_dice':
            v = c / (dr + dc).astype(np.float64)
            v = v * 2.
        elif sim == 'asymmetric_cosine':
            pa, p1a = np.power(deg, alpha), np.power(deg, 1 - alpha)
            v = c / (pa[rows][:, None] * p1a[None, :])
        elif sim == 'tversky':
            v = c / (c + alpha * (dr - counts).astype(np.float64) + beta * (dc - counts).astype(np.float64))
        else:
            raise ValueError(sim)
        f = c / (c + shrinkage)
    return v * f


def neighbours(M, sim, k, shrinkage, alpha=None, beta=None, block=2048):
    """CSR (indptr, indices, data) of the k nearest neighbours of each row of the entity matrix M (dense 0/1),
    rows in order (value desc, index asc); self and zero counts excluded."""
    n = M.shape[0]
    deg = M.sum(1).astype(np.int64)
    ptr, idx, val = [0], [], []
    for r0 in range(0, n, block):
        rows = np.arange(r0, min(r0 + block, n))
        counts = np.rint(M[rows] @ M.T).astype(np.int64)
        s = similarity_rows(counts, rows, deg, sim, shrinkage, alpha, beta)
        for t, r in enumerate(rows):
            cand = np.flatnonzero(counts[t] > 0)
            cand = cand[cand != r]
            order = np.lexsort((cand, -s[t, cand]))[:k]
            idx.append(cand[order])
            val.append(s[t, cand[order]])
            ptr.append(ptr[-1] + len(order))
    return (np.array(ptr, np.int64), np.concatenate(idx).astype(np.int32) if idx else np.zeros(0, np.int32),
            np.concatenate(val) if val else np.zeros(0))


def score_rows(users, a_csr, b_csr, n_cols):
    """row q = sum over A-row users[q] in stored order of w_a * B-row, from 0.0 (scipy's csr @ csr order).
    a_csr / b_csr = (indptr, indices, data or None)."""
    ap, ai, av = a_csr
    bp, bi, bv = b_csr
    out = np.zeros((len(users), n_cols))
    for q, u in enumerate(users):
        acc = out[q]
        for e in range(ap[u], ap[u + 1]):
            r, wa = ai[e], (1. if av is None else av[e])
            cols = bi[bp[r]:bp[r + 1]]
            wb = np.ones(len(cols)) if bv is None else bv[bp[r]:bp[r + 1]]
            acc[cols] = acc[cols] + wa * wb
    return out


def transpose(indptr, indices, data, n_rows, n_cols):
    rows = np.repeat(np.arange(n_rows), np.diff(indptr))
    order = np.lexsort((rows, indices))
    tp = np.zeros(n_cols + 1, np.int64)
    np.cumsum(np.bincount(indices, minlength=n_cols), out=tp[1:])
    return tp, rows[order].astype(np.int32), None if data is None else data[order]


def predictions(alg, users, x_csr, s_csr, n_users, n_items):
    """pred rows of `users`: iknn X S^T, uknn S X.  x_csr = (indptr, indices), s_csr = (indptr, indices, data)."""
    if alg == 'iknn':
        return score_rows(users, (*x_csr, None), transpose(*s_csr, n_items, n_items), n_items)
    return score_rows(users, s_csr, (*x_csr, None), n_items)


def masked_topk(pred, excl_rows, k=100):
    """(values, ids) of the k largest of each row after -inf on excl_rows[q] (list of column arrays)."""
    m = pred.copy()
    for q, cols in enumerate(excl_rows):
        m[q, cols] = -np.inf
    ids = np.stack([np.lexsort((np.arange(m.shape[1]), -row))[:k] for row in m])
    return np.take_along_axis(m, ids, 1), ids


def rank_metrics(ids, label_rows, ks=(5, 10, 50, 100)):
    """{name@k: [R]} precision / recall / ndcg of ranked ids against label_rows (eval/metrics.py definitions)."""
    out = {}
    for k in ks:
        rel = np.array([np.isin(ids[q, :k], label_rows[q]) for q in range(len(ids))], np.float64)
        n_rel = np.array([len(x) for x in label_rows], np.float64)
        disc = 1. / np.log2(np.arange(2, k + 2))
        idcg = np.array([disc[:min(k, int(n))].sum() for n in n_rel])
        out[f'precision@{k}'] = rel.sum(1) / k
        out[f'recall@{k}'] = np.where(n_rel > 0, rel.sum(1) / np.maximum(n_rel, 1), 0.)
        out[f'ndcg@{k}'] = np.minimum(np.where(idcg > 0, (rel * disc).sum(1) / np.maximum(idcg, 1e-30), 0.), 1.)
    return out
