"""numpy fp64 restatement of the calibration decorator's arithmetic (reference eval/eval.py:164-208 with
eval/metrics.py:108-152), the yardstick of hsk_calibration_metrics in tests/test_calibration.py.

Per row, with p = user_mtx[user] and the item rows added in rank order (an id outside [0, n_items) adds a zero row):
    q_k  = beta p + (1 - beta) (sum over rank < k of item_mtx[id_rank]) / k
    hel2 = .5 sum (sqrt p - sqrt q)^2                                  hellinger = sqrt(hel2)
    kl   = sum p (log p - log q)
    js2  = .5 (sum p (log p - log m) + sum q (log q - log m)), m = .5 (p + q)     js = sqrt(js2)
Nothing is guarded: log 0 = -inf, 0 * inf = NaN and NaN inputs go through as IEEE arithmetic has them.

Next to each compared quantity (hel2, js2, kl) comes its scale S, the size of what was added up to get it:
    S_hel2 = hel2,  S_kl = sum p (|log p| + |log q|),  S_js2 = .5 (sum p (|log p| + |log m|) + sum q (|log q| + |log m|))
so that a device result is held to |dev - restate| <= C 2^-52 S."""
import numpy as np

NAMES = ('hellinger_distance', 'jensen_shannon_distance', 'kl_divergence')


def smoothed_lists(ids, users, item_mtx, user_mtx, beta, ks):
    """(p [R, n_bins], q [len(ks), R, n_bins]) in fp64."""
    ids = np.asarray(ids, np.int64)
    item = np.asarray(item_mtx, np.float64)
    p = np.asarray(user_mtx, np.float64)[np.asarray(users, np.int64)]
    inside = (ids >= 0) & (ids < item.shape[0])
    rows = item[np.where(inside, ids, 0)] * inside[:, :, None]          # [R, k_max, n_bins]; pads are zero rows
    running = np.cumsum(rows, axis=1)                                   # sequential along the ranks
    q = np.stack([beta * p + (1 - beta) * (running[:, k - 1] / k) for k in ks])
    return p, q


def _kl(a, b):
    """(sum a (log a - log b), sum a (|log a| + |log b|)) over the last axis"""
    la, lb = np.log(a), np.log(b)
    return (a * (la - lb)).sum(-1), (a * (np.abs(la) + np.abs(lb))).sum(-1)


def calibration(ids, users, item_mtx, user_mtx, beta, ks):
    """-> dict of [R, len(ks), 3] fp64 arrays, last axis (hellinger, jensen-shannon, kl):
    'value' the three metrics, 'compared' (hel2, js2, kl), 'scale' their S."""
    with np.errstate(all='ignore'):
        p, q = smoothed_lists(ids, users, item_mtx, user_mtx, beta, ks)
        p = np.broadcast_to(p, q.shape)
        hel2 = .5 * ((np.sqrt(p) - np.sqrt(q)) ** 2).sum(-1)
        kl, s_kl = _kl(p, q)
        m = .5 * (p + q)
        kl_pm, s_pm = _kl(p, m)
        kl_qm, s_qm = _kl(q, m)
        js2 = .5 * (kl_pm + kl_qm)
        s_js2 = .5 * (s_pm + s_qm)
        out = {'value': np.stack([np.sqrt(hel2), np.sqrt(js2), kl], -1),
               'compared': np.stack([hel2, js2, kl], -1),
               'scale': np.stack([hel2, s_js2, s_kl], -1)}
    return {name: np.ascontiguousarray(np.swapaxes(a, 0, 1)) for name, a in out.items()}


def compared_of(values):
    """the compared quantities of a [.., 3] array of metrics: hellinger and js squared, kl as it is"""
    out = np.array(values, np.float64, copy=True)
    with np.errstate(all='ignore'):
        out[..., :2] **= 2
    return out


def metric_dict(ids, users, item_mtx, user_mtx, beta, ks, prefix):
    """per-user metrics under the decorator's names: '{prefix}_{name}@{k}' -> [R]"""
    val = calibration(ids, users, item_mtx, user_mtx, beta, ks)['value']
    return {f'{prefix}_{name}@{k}': val[:, t, j] for t, k in enumerate(ks) for j, name in enumerate(NAMES)}
