"""numpy-only restatement of the ranked half of every evaluation (no tests here): the order law of the fp64 selection
(`knn_key` / `knn_block_topk` of csrc/hsk_knn.hip) and the rank metrics of eval/metrics.py in float64 -- the expected
values of tests/test_rank_tail.py, which also holds this file to knn_restate, the g5 golden and the torch functions.

Order law: a double is ranked by its bit pattern, not by `<`: sign clear -> bit 63 set, sign set -> all bits
complemented, larger key first, ties to the lower index.  On finite non-zero doubles and +-inf that is `<`; beyond it,
-0.0 ranks below +0.0, a NaN with the sign bit clear above +inf and a NaN with the sign bit set below -inf."""
import numpy as np

SIGN = np.uint64(1 << 63)
PAD_ID = 0x7fffffff              # the id of a list entry that stands for nothing (hsk_topk_merge)


def key64(x):
    """uint64 keys of float64 values: larger key <=> ranked first."""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where((u & SIGN) != 0, ~u, u | SIGN)


def bits64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def topk64(S, k, valid=None):
    """(ids int64 [R, k], bits uint64 [R, k]) of the k first of each row of S in the order (key desc, index asc),
    among the columns where `valid` [R, n] (bool, default all) holds.  A row with fewer than k valid columns is
    filled up with id -1 and the bits of +0.0."""
    S = np.ascontiguousarray(S, dtype=np.float64)
    R, n = S.shape
    ids = np.full((R, k), -1, dtype=np.int64)
    out = np.zeros((R, k), dtype=np.uint64)
    for q in range(R):
        cand = np.arange(n) if valid is None else np.flatnonzero(valid[q])
        key = key64(S[q, cand])
        order = cand[np.lexsort((cand, ~key))[:k]]         # ascending in ~key = descending in key
        ids[q, :len(order)] = order
        out[q, :len(order)] = bits64(S[q, order])
    return ids, out


def discounts(k):
    return 1. / np.log2(np.arange(2, k + 2, dtype=np.float64))


def rank_metrics64(ids, label_rows, ks):
    """eval/metrics.py in float64, from ranked ids [R, k_max] and label_rows[q] (the user's relevant ids, distinct).
    Counted per position: a duplicated id counts wherever it stands (torch.gather); an id in no label row never hits.
    -> dict(hits int64 [R, T], n_rel int64 [R], metrics float64 [R, T, 3] = precision, recall, ndcg at ks[t])."""
    ids = np.asarray(ids, dtype=np.int64)
    R = ids.shape[0]
    n_rel = np.array([len(x) for x in label_rows], dtype=np.int64)
    hit = np.stack([np.isin(ids[q], np.asarray(label_rows[q], dtype=np.int64)) for q in range(R)]) if R else \
        np.zeros(ids.shape, bool)
    disc = discounts(ids.shape[1])
    hits = np.zeros((R, len(ks)), dtype=np.int64)
    met = np.zeros((R, len(ks), 3))
    for t, k in enumerate(ks):
        h = hit[:, :k].sum(1)
        dcg = (hit[:, :k] * disc[:k]).sum(1)
        idcg = np.array([disc[:min(k, int(m))].sum() for m in n_rel])
        hits[:, t] = h
        met[:, t, 0] = h / k
        met[:, t, 1] = np.where(n_rel > 0, h / np.maximum(n_rel, 1), 0.)
        met[:, t, 2] = np.where(n_rel > 0, np.minimum(dcg / np.where(idcg > 0, idcg, 1.), 1.), 0.)
    return dict(hits=hits, n_rel=n_rel, metrics=met)


def f32_ratio(num, den):
    """float32(num) / float32(den), correctly rounded: what precision and recall must be bit for bit."""
    return np.asarray(num, dtype=np.float32) / np.asarray(den, dtype=np.float32)


def ndcg_c(k, log2_ulp=2):
    """The number c of 2^-24 relative roundings between the kernel's float32 ndcg@k and the float64 value.  Per term of a
    sum: log2f (log2_ulp ulp, one ulp being at most 2^-23 of the value, so 2 log2_ulp units) and the correctly rounded
    reciprocal (1).  Per sum of positive terms: ceil(k / 64) - 1 additions in a lane and 6 in the wave's tree, each at most
    one unit of the partial sum.  DCG and IDCG each carry that, and the final division one more."""
    per_sum = 2 * log2_ulp + 1 + (-(-k // 64) - 1) + 6
    return 2 * per_sum + 1
