"""The cases of tests/test_unfused_ops.py as plain numpy data: shapes, index arrays and tables, built on the host from
seeds, so that tests/test_ops_restate.py can check their claims (exactness precondition, coverage of the dispatch
boundaries) without a GPU.

The boundaries the grids are built around (csrc/hsk_ops.hip, csrc/hsk_rows.h):
  columns    a wave owns 128 columns in two passes of 64, a workgroup 512; a second workgroup along x exists from
             K = 513; rows of a pass are buffered R at a time (R = 2 when V * NCH >= 16, else 4) with a guarded remainder
  row shape  tile(D) = (V, NCH, FULL); refused just past 512 / 1024 / 2048 for V = 1 / 2 / 4
  batch      scores are cut into launches of 65 535 rows, the backward passes refuse more
"""
import zlib

import numpy as np

import ops_restate as R

N_USERS, N_ITEMS = 37, 53
SPARE_USER, SPARE_ITEMS = 1, (1, N_ITEMS - 2)      # rows no valid index names: their gradients must stay zero

K_LADDER = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 193, 511, 512, 513, 1025)
K_LADDER_B = (1, 4, 5)
K_LADDER_D = (64, 1024)                            # R = 4 and R = 2
D_V1 = (1, 2, 3, 63, 65, 127, 129, 255, 257, 511)  # (2 is served as one V = 2 chunk: it is even)
D_V2 = (6, 126, 130, 254, 258, 402, 1022)
D_V4 = (4, 60, 252, 256, 260, 508, 512, 1020, 1024, 1028, 2044, 2048)
D_LADDER = D_V1 + D_V2 + D_V4
D_LADDER_K = (5, 129)
D_REFUSED = (513, 1026, 2052)
BIAS_SETS = tuple((bool(m & 1), bool(m & 2), bool(m & 4)) for m in range(8))   # (item, user, global)
BIAS_K, BIAS_D = (3, 129), (30, 256)
DUP_KINDS = ('item_row', 'same_user', 'pos_eq_neg', 'last_row')
DUP_K = (129, 513)
BAD_VALUES = ('-1', 'n', '2^40')
BAD_K = 130
BAD_COLS = (0, 63, 64, 127, 128, BAD_K - 1)
BATCH_LIMIT = dict(B=65538, K=3, D=4)
BIAS_LADDER_B = (1, 5, 9)
EMB_N = (1, 3, 4, 5, 1025)


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()))


def _bad_value(tag, n):
    return {'-1': -1, 'n': n, '2^40': 1 << 40}[tag]


def make_case(name, D, B, K, bias=(True, True, True), kind='random', bad=None, n_users=N_USERS, n_items=N_ITEMS):
    """-> dict(name, D, B, K, bias, n_users, n_items, u [B], i [B, K] int64 -- as handed to the operator, bad entries
    included --, bad).  bad = (which in 'u' / 'i', value tag, row, column)."""
    rng = _rng(name)
    users = np.array([x for x in range(n_users) if x != SPARE_USER])
    items = np.array([x for x in range(n_items) if x not in SPARE_ITEMS])
    u = users[rng.randint(0, len(users), size=B)].astype(np.int64)
    i = items[rng.randint(0, len(items), size=(B, K))].astype(np.int64)
    if kind == 'item_row':        # every column of a row the same item
        i[:] = i[:, :1]
    elif kind == 'same_user':     # every row the same user
        u[:] = u[0]
    elif kind == 'pos_eq_neg':    # the positive once more among the negatives (last column; K == 1 has none)
        i[:, -1] = i[:, 0]
    elif kind == 'last_row':      # the tables' last rows: every user, every second column
        u[:] = n_users - 1
        i[:, ::2] = n_items - 1
    elif kind != 'random':
        raise ValueError(kind)
    if bad is not None:
        which, tag, row, col = bad
        if which == 'u':
            u[row] = _bad_value(tag, n_users)
        else:
            i[row, col] = _bad_value(tag, n_items)
    return dict(name=name, D=D, B=B, K=K, bias=tuple(bias), n_users=n_users, n_items=n_items, u=u, i=i, bad=bad,
                kind=kind)


def tables(case, mode):
    """-> dict of float32 arrays: user_emb / item_emb ([rows, D]; None when D == 0), item_bias, user_bias, global_bias
    (None where the case has none; dim == 0 always has the two tables) and grad [B, K].
    mode 'exact': tables integers in [-8, 8], biases in [-16, 16], grad in [-4, 4]; 'rounded': randn * 0.3, randn * 0.1
    and randn."""
    rng = _rng(case['name'] + '/' + mode)
    nu, ni, D = case['n_users'], case['n_items'], case['D']
    has_ib, has_ub, has_gb = case['bias']
    if D == 0:
        has_ib = has_ub = True

    def table(shape, int_bound, sigma):
        if mode == 'exact':
            return rng.randint(-int_bound, int_bound + 1, size=shape).astype(np.float32)
        return (rng.randn(*shape) * sigma).astype(np.float32)

    T = {'user_emb': table((nu, D), 8, 0.3) if D else None, 'item_emb': table((ni, D), 8, 0.3) if D else None,
         'item_bias': table((ni,), 16, 0.1), 'user_bias': table((nu,), 16, 0.1), 'global_bias': table((1,), 16, 0.1),
         'grad': table((case['B'], case['K']), 4, 1.0)}
    if case['bad'] is not None and mode == 'exact':
        # the bad entry must show wherever it lands: its gradient is not zero, and row 0 of the bias tables (what the
        # clamp reads) differs from their last row (what an off-by-one clamp would read)
        which, _, row, col = case['bad']
        g = T['grad'][row] if which == 'u' else T['grad'][row, col:col + 1]
        g[g == 0] = 3.0
        for k, a, b in (('item_bias', 5.0, -7.0), ('user_bias', 4.0, -6.0)):
            T[k][0], T[k][-1] = a, b
    for k, has in (('item_bias', has_ib), ('user_bias', has_ub), ('global_bias', has_gb)):
        if not has:
            T[k] = None
    return T


def expected(case, T):
    """The restatement on the clamped indices -> (scores (s, scale, n), grads {name: (grad, scale, n)}, status word)."""
    uc, ic = R.clamp(case['u'], case['n_users']), R.clamp(case['i'], case['n_items'])
    sc = R.scores(T['user_emb'], T['item_emb'], T['item_bias'], T['user_bias'], T['global_bias'], uc, ic)
    gr = R.backward(T['user_emb'], T['item_emb'], uc, ic, T['grad'], case['n_users'], case['n_items'])
    status = 1 if R.is_bad(case['u'], case['n_users']) or R.is_bad(case['i'], case['n_items']) else 0
    return sc, gr, status


# ------------------------------------------------------------------------------------------------
# the grids (crossed sparsely: each axis in full, the others cycling)
# ------------------------------------------------------------------------------------------------
def k_ladder_cases():
    out = []
    for d, D in enumerate(K_LADDER_D):
        for j, K in enumerate(K_LADDER):
            B = K_LADDER_B[(j + d) % 3]
            out.append(make_case(f'k{K}-b{B}-d{D}', D, B, K))
    return out


def d_ladder_cases():
    out = []
    for j, D in enumerate(D_LADDER):
        for k, K in enumerate(D_LADDER_K):
            B = K_LADDER_B[(j + k) % 3]
            out.append(make_case(f'd{D}-k{K}-b{B}', D, B, K))
    return out


def _bias_tag(bias):
    return ''.join(c for c, has in zip('iug', bias) if has) or 'none'


def bias_set_cases():
    return [make_case(f'bias-{_bias_tag(bias)}-k{K}-d{D}', D, 4, K, bias=bias)
            for bias in BIAS_SETS for K in BIAS_K for D in BIAS_D]


def dup_cases(D=64):
    return [make_case(f'dup-{kind}-k{K}-d{D}', D, 64 if kind == 'same_user' else 5, K, kind=kind)
            for kind in DUP_KINDS for K in DUP_K]


def bad_cases(D=64):
    out = []
    for tag in BAD_VALUES:
        out.append(make_case(f'bad-u-{tag}-d{D}', D, 5, BAD_K, bad=('u', tag, 2, 0)))
        for j, col in enumerate(BAD_COLS):
            out.append(make_case(f'bad-i-{tag}-c{col}-d{D}', D, 5, BAD_K, bad=('i', tag, j % 5, col)))
    return out


def mf_cases():
    return k_ladder_cases() + d_ladder_cases() + bias_set_cases() + dup_cases() + bad_cases()


def bias_ladder_cases():
    out = []
    for g, has_gb in enumerate((True, False)):
        for j, K in enumerate(K_LADDER):
            B = BIAS_LADDER_B[(j + g) % 3]
            out.append(make_case(f'k{K}-b{B}-{"gb" if has_gb else "nogb"}-d0', 0, B, K, bias=(True, True, has_gb)))
    return out


def bias_cases():
    return bias_ladder_cases() + dup_cases(D=0) + bad_cases(D=0)


def batch_limit_case(D=BATCH_LIMIT['D']):
    return make_case(f'batch-limit-d{D}', D, BATCH_LIMIT['B'], BATCH_LIMIT['K'])


def embedding_cases():
    """(D, n, shape of idx): every D of the ladder, n cycling; the (7, 3) shape for every fourth."""
    out = []
    for j, D in enumerate(D_LADDER):
        out.append((D, EMB_N[j % len(EMB_N)], (7, 3) if j % 4 == 3 else None))
    for n in EMB_N:
        out.append((64, n, None))
    return out


# ------------------------------------------------------------------------------------------------
# what the grids claim to reach, computed from the launch geometry the operators document
# ------------------------------------------------------------------------------------------------
WAVE_COLS, GROUP_COLS, PASS_COLS = 128, 512, 64


def column_geometry(K, D):
    """What a [*, K] call at dimension D exercises: workgroups along x, waves that retire (k0 >= K) in the last
    workgroup, the sizes of the ragged passes, and the remainders of those against R."""
    Rbuf = R.score_rows_buffered(D)
    groups = -(-K // GROUP_COLS)
    live_waves = -(-K // WAVE_COLS)
    passes = [min(PASS_COLS, K - k) for k in range(0, K, PASS_COLS)]
    return dict(R=Rbuf, groups=groups, retired_waves=groups * 4 - live_waves, passes=passes,
                remainders={nr % Rbuf for nr in passes})


def coverage(cases):
    """-> dict of the sets a list of cases reaches."""
    tiles = {R.tile(c['D']) for c in cases if c['D'] > 0}
    residues = {(column_geometry(c['K'], c['D'])['R'], c['K'] % 4) for c in cases if c['D'] > 0}
    remainders = set()
    for c in cases:
        if c['D'] > 0:
            g = column_geometry(c['K'], c['D'])
            remainders |= {(g['R'], r) for r in g['remainders']}
    return dict(tiles=tiles, residues=residues, remainders=remainders,
                second_group=any(c['K'] > GROUP_COLS for c in cases if c['D'] > 0),
                retired_waves=any(column_geometry(c['K'], c['D'])['retired_waves'] > 0 for c in cases if c['D'] > 0),
                ragged_y=any(c['B'] % 4 for c in cases))


ALL_TILES = {(V, NCH) for V in (1, 2, 4) for NCH in (1, 2, 4, 8)}
