"""Builders shared by tests/test_eval_structured.py and tools/stress_eval.py (no tests here): integer score tables
with a prescribed structure along the item id, whose scores are exact in every arithmetic form, and the exact numpy
top-k they must give."""
import numpy as np

B_SHAPES = {   # name: (rows, n_users, n_items, D, k, (item_begin, item_count) of the range run)
    'seeded-17000': (300, 320, 17000, 64, 100, (300, 16500)),      # >= 16384 items: seeded thresholds, splits, the merge
    'long-40000': (70, 70, 40000, 16, 128, (1000, 38900)),         # one row block, many splits
    'mid-5000': (257, 400, 5000, 512, 5, (123, 4700)),             # forms 0 / 1: the 128 x 128 kernel with S > 1; rows 257
    'one-split-300': (130, 200, 300, 64, 1, (10, 277)),            # a single split, rows ragged against 128
    'two-tiles-129': (64, 64, 129, 16, 100, (20, 105)),            # the second tile holds one column; the range: one tile
}
B_KINDS = [('rising', False), ('rising', True), ('falling', True), ('saw_up', True), ('saw_down', False),
           ('quantised', False), ('quantised', True), ('equal', False), ('equal', True), ('hidden', True),
           ('last_tile', False), ('last_tile', True)]
B_SEED_COLS = 4096


def item_pattern(kind, cnt, rng):
    """Integer rank pattern p[j], j = column of the scored window; the item bias is 1.5 p."""
    j = np.arange(cnt)
    T = (cnt + 255) // 256
    if kind == 'rising':
        return j
    if kind == 'falling':
        return cnt - 1 - j
    if kind == 'saw_up':        # rises inside each 256-column tile, falls from tile to tile
        return (T - 1 - j // 256) * 256 + j % 256
    if kind == 'saw_down':      # falls inside each tile, rises from tile to tile
        return (j // 256) * 256 + 255 - j % 256
    if kind == 'quantised':
        return rng.randint(0, 4, size=cnt)
    if kind == 'equal':
        return np.zeros(cnt, dtype=np.int64)
    if kind == 'hidden':
        return rng.randint(0, 1000, size=cnt)
    assert kind == 'last_tile'  # a few values everywhere, the winners in the last (ragged) tile of the last split
    p = rng.randint(0, 4, size=cnt)
    w = cnt - (T - 1) * 256
    p[cnt - w:] = 100 + rng.permutation(w)
    return p


def selection_case(shape, kind, hard_excl, lo, cnt, seed=0):
    """Integer tables, half-integer biases, an exclusion CSR and the exact float64 scores of the window [lo, lo + cnt)."""
    R, n_users, n_items, D, k, _ = shape
    rng = np.random.RandomState(seed + 1000 * len(kind) + n_items + lo)
    noisy = kind not in ('quantised', 'equal')
    V = rng.randint(-8, 8, size=D)
    I = np.tile(V, (n_items, 1))
    if noisy:                        # one column differs from item to item by 0 / 1: less than a bias step of 1.5
        I[:, 0] += rng.randint(0, 2, size=n_items)
    U = rng.randint(-8, 9, size=(n_users, D))
    U[:, 0] = rng.randint(-1, 2, size=n_users)
    p = np.full(n_items, 50000, dtype=np.int64)     # outside the window: would win if a kernel looked there
    p[lo:lo + cnt] = item_pattern(kind, cnt, rng)
    Ib = None if kind == 'equal' else 1.5 * p
    Ub = None if kind in ('equal', 'quantised') else 0.5 * rng.randint(-50, 50, size=n_users)
    gb = None if kind in ('equal', 'quantised') else np.array([3.5])
    u = rng.randint(0, n_users, size=R)
    u[:min(4, R)] = np.arange(min(4, R))
    U64, I64 = U[u].astype(np.float64), I[lo:lo + cnt].astype(np.float64)    # (integers: exact in float64)
    S = U64 @ I64.T
    mag = np.abs(U64) @ np.abs(I64).T
    for b in ((None if Ub is None else Ub[u][:, None]), (None if Ib is None else Ib[lo:lo + cnt][None, :]), gb):
        if b is not None:
            S = S + b
            mag = mag + np.abs(b)
    # the premise: every score and every partial sum is an integer or half-integer below 2^24 -- exact in fp32
    assert mag.max() < 2 ** 24 and np.array_equal(2 * S, np.round(2 * S))
    for b in (Ib, Ub, gb):
        assert b is None or (np.abs(b).max() < 2 ** 20 and np.array_equal(2 * b, np.round(2 * b)))
    pairs = None
    if hard_excl:
        win = np.arange(lo, lo + cnt)
        best = lo + np.argsort(-S[0], kind='stable')[:k]                 # user 0: its k best are all excluded
        head = win[:B_SEED_COLS]
        few = head[::max(1, len(head) // max(k - 3, 1))][:max(k - 3, 0)]     # user 1: k - 3 admissible in the seeded sample
        out1 = np.setdiff1d(np.arange(0, min(n_items, lo + B_SEED_COLS)), few)
        out2 = np.setdiff1d(np.arange(n_items), win[::7][:max(k - 2, 0)])    # user 2: k - 2 admissible overall
        parts = [np.stack([np.full(len(x), uu), x], 1) for uu, x in ((0, best), (1, out1), (2, out2), (3, np.arange(n_items)))]
        others = np.arange(4, n_users)
        parts.append(np.stack([np.repeat(others, 30), rng.randint(0, n_items, size=30 * len(others))], 1))
        even = others[others % 2 == 0]                                   # ... and some of the window's first ids
        parts += [np.stack([even, np.full(len(even), lo + c)], 1) for c in (0, 2, 3) if c < cnt]
        pairs = np.concatenate(parts)
    return dict(U=U.astype(np.float32), I=I.astype(np.float32), Ib=None if Ib is None else Ib.astype(np.float32),
                Ub=None if Ub is None else Ub.astype(np.float32), gb=None if gb is None else gb.astype(np.float32),
                u=u.astype(np.int64), S=S, pairs=pairs, n_users=n_users, k=k, lo=lo, cnt=cnt)


def expected_topk(S, pairs, u, k, lo, lowest_id_first=True):
    """Exact top-k of the masked scores: (values float32, ids int32), score descending, then id ascending; rows with fewer
    than k admissible items fill up with -inf entries, lowest id first."""
    S = S.copy()
    cnt = S.shape[1]
    if pairs is not None:
        excl = np.zeros((int(u.max()) + 1, cnt), dtype=bool)
        m = (pairs[:, 1] >= lo) & (pairs[:, 1] < lo + cnt) & (pairs[:, 0] <= u.max())
        excl[pairs[m, 0], pairs[m, 1] - lo] = True
        S[excl[u]] = -np.inf
    if lowest_id_first:
        order = np.argsort(-S, axis=1, kind='stable')[:, :k]
    else:
        order = cnt - 1 - np.argsort(-S[:, ::-1], axis=1, kind='stable')[:, :k]
    return np.take_along_axis(S, order, 1).astype(np.float32), (order + lo).astype(np.int32)


def bits(v):
    """float32 values as their bit patterns, -0.0 counted as 0.0 (a sum that cancels may carry either sign)."""
    return (np.asarray(v, dtype=np.float32) + np.float32(0.0)).view(np.int32)
