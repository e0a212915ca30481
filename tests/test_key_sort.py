"""The three item sorts of csrc/hsk_sort.h (k_sort_lds, k_sort_small<2|4|8>, the two-level sort) held to numpy's stable
argsort at every size threshold of the dispatch rule, through the debug entry hsk_key_sort -- the same hsk_launch_sort
every training step, hsk_embedding_backward and hsk_sparse_rows_sum_backward go through.

Every comparison here is exact: perm / offsets / touched are integers, and the operators' gradients are compared bit for
bit with an fp32 sum that adds the rows one at a time in stable-sort order (ascending position inside a key).  The
payload of those sums is made so that the order shows: its terms span 25 binades with both signs, so adding a key's
list in another order changes the rounding (test_payload_reveals_the_summation_order checks that it does).

CASES names one shape per threshold.  The CPU tests pin what hsk_key_sort_plan answers for each, so that moving a
threshold breaks a named case here instead of silently moving a kernel out of the GPU tests' reach.
"""
import functools

import numpy as np
import pytest
import torch

from test_dmf import N_IN, ROW_LENGTHS, _hand_csr

LDS_MAX = 163840   # bytes of LDS one workgroup can have on gfx950

# (n_keys, n, kind, expected plan fields, what the case is there for)
CASES = [
    (2048, 8192, 'lds', dict(lds_bytes=90368), 'k_sort_lds at its entry limit, 4 entries per key: the densest it takes'),
    (2047, 8192, 'small8', dict(nbits=11), 'one key fewer: k_sort_small<8>, every thread full (no padding key)'),
    (8000, 8192, 'lds', dict(lds_bytes=161792), 'k_sort_lds at its key limit: the largest LDS request it makes'),
    (8001, 8192, 'small8', dict(nbits=13), 'one key more: k_sort_small<8> without padding, 13 radix bits'),
    (8000, 8193, 'two_level', dict(shift=4, n_buckets=500, ipb=16, epw=1024, n_units=9),
     'one entry more: two-level, 9 units = dead waves in the last workgroup of hist / scatter'),
    (500, 2048, 'small2', dict(nbits=9), 'k_sort_small<2> without padding'),
    (500, 2049, 'small4', dict(nbits=9), 'one entry more: k_sort_small<4>'),
    (1000, 4096, 'small4', dict(nbits=10), 'k_sort_small<4> without padding'),
    (1000, 4097, 'small8', dict(nbits=10), 'one entry more: k_sort_small<8>'),
    (1, 9000, 'two_level', dict(shift=0, n_buckets=1, ipb=1, epw=1024, n_units=9),
     'one bucket of one key: hsk_match_any over 0 bits in both levels'),
    (512, 9000, 'two_level', dict(shift=0, n_buckets=512, ipb=1), 'as many buckets as there can be, one key each'),
    (513, 9000, 'two_level', dict(shift=1, n_buckets=257, ipb=2), 'ragged last bucket: it holds one key of its two'),
    (100000, 70000, 'two_level', dict(shift=8, n_buckets=391, ipb=256, epw=1024, n_units=69),
     '69 units: not a multiple of the 4 waves of a workgroup; ragged last bucket'),
    (5000, 524288, 'two_level', dict(epw=1024, n_units=512), 'as many units as there can be, 1024 entries each'),
    (5000, 524289, 'two_level', dict(epw=2048, n_units=257), 'one entry more: units of 2048 = the g0 != lo reload loops'),
    (2097152, 20000, 'two_level', dict(shift=12, n_buckets=512, ipb=4096, lds_bytes=81920),
     'the most keys a sort with a touched list takes'),
    (2097153, 20000, 'two_level', dict(shift=13, n_buckets=257, ipb=8192, lds_bytes=163840),
     'buckets of 8192 keys: level 2 asks for all the LDS of a workgroup; ragged last bucket of one key'),
    (4194304, 20000, 'two_level', dict(shift=13, n_buckets=512, ipb=8192, lds_bytes=163840), 'the most keys any sort takes'),
    (4194305, 20000, 'unsupported', dict(), 'one key more'),
]
# with a touched list (lazy_items) the level-2 counters are 6 * ipb + 2 ints: buckets of 8192 keys do not fit
TOUCHED_UNSUPPORTED = {2097153, 4194304, 4194305}
EXTRA_CASES = [   # n = 1: every kernel with a single live lane
    (1, 1, 'lds', dict(), 'one entry, one key'),
    (2048, 1, 'lds', dict(), 'one entry'),
    (8001, 1, 'small2', dict(), 'one entry through the block radix sort: 2047 padding keys'),
]
IPT = {'small2': 2, 'small4': 4, 'small8': 8}
NO_PADDING = {(2047, 8192), (8001, 8192), (500, 2048), (1000, 4096)}   # n == 1024 * IPT: thread 1023 closes offsets


def _id(case):
    return f'{case[0]}x{case[1]}'


def _plan(n_keys, n, touched=False):
    from hassaku_amd import hip_ops
    return hip_ops.key_sort_plan(n_keys, n, touched)


# ------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize('case', CASES + EXTRA_CASES, ids=_id)
def test_plan_table(case):
    """hsk_key_sort_plan sends each case to the kernel its comment names, with the plan it names."""
    from hassaku_amd import _lib
    n_keys, n, kind, fields, why = case
    plan = _plan(n_keys, n)
    assert plan['kind'] == kind, (why, plan)
    for k, v in fields.items():
        assert plan[k] == v, (why, k, plan)
    if kind in IPT:
        assert n <= 1024 * IPT[kind] and (IPT[kind] == 2 or n > 512 * IPT[kind]), (why, plan)
        assert ((n_keys, n) in NO_PADDING) == (n == 1024 * IPT[kind]), why
        assert (1 << plan['nbits']) > n_keys >= (1 << (plan['nbits'] - 1)), (why, plan)    # the padding key n_keys fits
        assert plan['lds_bytes'] == 0 and plan['n_units'] == 0
    if kind == 'two_level':
        assert plan['ipb'] == 1 << plan['shift'] and plan['n_buckets'] == ((n_keys - 1) >> plan['shift']) + 1 <= 512
        assert plan['epw'] % 1024 == 0 and plan['n_units'] == -(-n // plan['epw']) <= 512
        assert plan['shift'] == 0 or ((n_keys - 1) >> (plan['shift'] - 1)) + 1 > 512      # the smallest such shift
        assert plan['epw'] == 1024 or -(-n // (plan['epw'] // 2)) > 512
    if kind == 'lds':
        assert n <= 8192 and n_keys <= 8000 and n <= 4 * n_keys
        assert plan['lds_bytes'] == (3 * n_keys + 2 * 8192 + 64) * 4
    lib = _lib.load()
    assert (lib.hsk_key_sort_ws_bytes(n_keys, n, 0) > 0) == (kind != 'unsupported')
    # with a touched list: the same sort, or none
    lazy = _plan(n_keys, n, True)
    if n_keys in TOUCHED_UNSUPPORTED:
        assert lazy['kind'] == 'unsupported' and lib.hsk_key_sort_ws_bytes(n_keys, n, 1) < 0
    else:
        assert lazy['kind'] == kind and lib.hsk_key_sort_ws_bytes(n_keys, n, 1) > lib.hsk_key_sort_ws_bytes(n_keys, n, 0)
        assert {k: v for k, v in lazy.items() if k != 'lds_bytes'} == {k: v for k, v in plan.items() if k != 'lds_bytes'}
        if kind == 'two_level':
            assert lazy['lds_bytes'] == (6 * lazy['ipb'] + 2) * 4 and plan['lds_bytes'] == 5 * plan['ipb'] * 4


def test_no_supported_shape_asks_for_more_lds_than_a_workgroup_has():
    """Whatever hsk_key_sort_plan supports, its launch fits: the table, and n_keys = 2^k, 2^k +- 1 for k = 0..22 at an
    entry count for each sort, with and without the touched list."""
    shapes = [(c[0], c[1]) for c in CASES + EXTRA_CASES]
    for k in range(23):
        for n_keys in (2 ** k - 1, 2 ** k, 2 ** k + 1):
            if n_keys >= 1:
                shapes += [(n_keys, n) for n in (1, 2048, 4096, 8192, 8193, 20000, 524289)]
    seen = set()
    for n_keys, n in shapes:
        for touched in (False, True):
            plan = _plan(n_keys, n, touched)
            seen.add((plan['kind'], touched))
            assert 0 <= plan['lds_bytes'] <= LDS_MAX, (n_keys, n, touched, plan)
            limit = 2097152 if touched else 4194304
            assert (plan['kind'] == 'unsupported') == (n_keys > limit), (n_keys, n, touched, plan)
    assert seen == {(kind, t) for kind in ('lds', 'small2', 'small4', 'small8', 'two_level', 'unsupported')
                    for t in (False, True)}


def test_the_library_refuses_a_state_the_item_sort_cannot_take():
    """hsk_bprmf_workspace_bytes (no lazy_items in its arguments) stops at the limit of the sort without a touched list."""
    from hassaku_amd import _lib
    lib = _lib.load()
    assert lib.hsk_bprmf_workspace_bytes(10, 4194304, 2, 8, 3) > 0
    assert lib.hsk_bprmf_workspace_bytes(10, 4194305, 2, 8, 3) < 0
    assert lib.hsk_embedding_backward_ws_bytes(4194304, 20000) > 0
    assert lib.hsk_embedding_backward_ws_bytes(4194305, 20000) < 0
    assert lib.hsk_sparse_rows_sum_backward_ws_bytes(4194305, 20000) < 0


# ---- payload and sequential reference of the operator tests
def _payload(n, dim, seed):
    """sign * (1 + U[0, 1)) * 2^randint(-12, 13): fp32 terms whose sum depends on the order they are added in."""
    rng = np.random.RandomState(seed)
    mag = (1 + rng.rand(n, dim)) * np.exp2(rng.randint(-12, 13, size=(n, dim)))
    return (np.where(rng.rand(n, dim) < 0.5, -1.0, 1.0) * mag).astype(np.float32)


def _stable_index(keys, n_keys):
    keys = np.asarray(keys)
    perm = np.argsort(keys, kind='stable').astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=n_keys))]).astype(np.int32)
    return perm, offsets


def _sequential_sums(keys, n_keys, rows, descending=False):
    """out[k] = ((0 + rows[p_0]) + rows[p_1]) + ... in fp32 over the positions p of key k, ascending (or descending):
    vectorised over the keys, a loop over the rank inside a key."""
    perm, offsets = _stable_index(keys, n_keys)
    count = np.diff(offsets)
    out = np.zeros((n_keys, rows.shape[1]), np.float32)
    for r in range(int(count.max())):
        sel = np.nonzero(count > r)[0]
        at = offsets[sel + 1] - 1 - r if descending else offsets[sel] + r
        out[sel] = out[sel] + rows[perm[at]]
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


EMB_CASES = [   # (n_keys, n, kind, dims): one per sort kind and more
    (2048, 8192, 'lds', (1, 6, 64)),
    (40, 1200, 'small2', (1, 6, 64)),
    (1000, 4096, 'small4', (1, 6, 64)),
    (2047, 8192, 'small8', (1, 6, 64)),
    (513, 9000, 'two_level', (1, 6, 64)),
    (5000, 524289, 'two_level', (1,)),     # the reload loops; 2 MB of gradient at dim 1
]
# batches over test_dmf's hand-made CSR: every row `reps` times (870 pairs per repetition); 0 stands for its seven
# rows of 1 .. 65 entries five times (1155 pairs) -- few enough pairs for k_sort_lds, in lists long enough to show order
CSR_REPS = [(0, 'lds'), (2, 'small2'), (4, 'small4'), (8, 'small8'), (12, 'two_level')]
CSR_DIMS = (1, 6, 64)


@functools.lru_cache(maxsize=None)
def _emb_keys(n_keys, n):
    return np.random.RandomState(n_keys + n).randint(0, n_keys, size=n).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _csr_batch(reps):
    """The rows of CSR_REPS[reps] in a seeded order -> (idx, the pairs' columns in pair order, the pairs' batch
    positions)."""
    indptr, indices, _ = _hand_csr()
    rows = np.tile(np.arange(len(ROW_LENGTHS)), reps) if reps else np.tile([1, 2, 3, 4, 8, 10, 11], 5)
    idx = np.random.RandomState(reps).permutation(rows).astype(np.int64)
    cols = np.concatenate([indices[indptr[r]:indptr[r + 1]] for r in idx]).astype(np.int64)
    pos = np.repeat(np.arange(len(idx)), [ROW_LENGTHS[r] for r in idx])
    return idx, cols, pos


def _operator_cases():
    for n_keys, n, kind, dims in EMB_CASES:
        for dim in dims:
            yield f'embedding {n_keys}x{n} dim {dim}', n_keys, _emb_keys(n_keys, n), _payload(n, dim, dim + n)
    for reps, kind in CSR_REPS:
        idx, cols, pos = _csr_batch(reps)
        for dim in CSR_DIMS:
            yield f'sparse_rows_sum x{reps} dim {dim}', N_IN, cols, _payload(len(idx), dim, dim + reps)[pos]


def test_operator_cases_take_every_sort():
    assert [_plan(k, n)['kind'] for k, n, _, _ in EMB_CASES] == [kind for _, _, kind, _ in EMB_CASES]
    assert [_plan(N_IN, len(_csr_batch(reps)[1]))['kind'] for reps, _ in CSR_REPS] == [kind for _, kind in CSR_REPS]
    assert {kind for _, kind in CSR_REPS} == {kind for _, _, kind, _ in EMB_CASES} == set(IPT) | {'lds', 'two_level'}


def test_payload_reveals_the_summation_order():
    """A condition of the operator tests, not a tolerance on the kernels: for at least a quarter of the keys with three
    or more entries, the fp32 sum in descending position differs bitwise from the sum in ascending position -- so a sort
    that grouped correctly but ordered a list wrongly would not pass them by luck."""
    for name, n_keys, keys, rows in _operator_cases():
        rows = rows[:, :1]
        up, down = _sequential_sums(keys, n_keys, rows), _sequential_sums(keys, n_keys, rows, descending=True)
        many = np.bincount(keys, minlength=n_keys) >= 3
        share = float((_bits(up)[many, 0] != _bits(down)[many, 0]).mean())
        print(f'{name}: {int(many.sum())} keys with >= 3 entries, {100 * share:.0f} % differ between the two orders')
        assert many.sum() >= 20 and share >= 0.25, (name, share)


# ------------------------------------------------------------------------------------------------------ GPU
DISTS = ('uniform', 'popular', 'last_key', 'key_0', 'descending', 'lists_8_9')


@functools.lru_cache(maxsize=2)
def _keys(n_keys, n, dist):
    rng = np.random.RandomState(n_keys % 9973 + n + DISTS.index(dist))
    if dist == 'uniform':
        keys = rng.randint(0, n_keys, size=n)
    elif dist == 'popular':           # 30 % of the entries on one key, every 16th ("one whole column") on another
        keys = rng.randint(0, n_keys, size=n)
        keys[rng.rand(n) < 0.3] = 3 % n_keys
        keys[::16] = 7 % n_keys
    elif dist == 'last_key':
        keys = np.full(n, n_keys - 1)
    elif dist == 'key_0':
        keys = np.zeros(n)
    elif dist == 'descending':
        keys = ((n - 1 - np.arange(n, dtype=np.int64)) * n_keys) // n
    else:
        # k_sort_lds: lists of exactly 8 (one thread, the exchange network) and exactly 9 entries (a wave, by rank) side
        # by side, one list longer than a wave, the rest anywhere else; positions shuffled
        keys = np.concatenate([np.repeat([0, 1, 2, 3, 4], [8, 9, 8, 9, 70]), rng.randint(5, n_keys, size=n - 104)])
        keys = keys[rng.permutation(n)]
    keys = keys.astype(np.int64)
    perm, offsets = _stable_index(keys, n_keys)
    return keys, perm, offsets


def _gpu_cases():
    for case in CASES + EXTRA_CASES:
        n_keys, n, kind = case[:3]
        for dist in DISTS:
            if dist == 'lists_8_9' and (kind != 'lds' or n < 1000):
                continue
            if kind == 'unsupported' and dist != 'uniform':
                continue
            yield pytest.param(n_keys, n, kind, dist, id=f'{n_keys}x{n}-{dist}')


@pytest.mark.gpu
@pytest.mark.parametrize('n_keys, n, kind, dist', list(_gpu_cases()))
def test_sort_is_the_stable_sort(n_keys, n, kind, dist):
    """perm == numpy's stable argsort and offsets == the prefix sums of the key counts, integer for integer; with the
    touched list the same perm / offsets and exactly the keys that have entries.  (n = 8192 entries on one key of
    2048 -- k_sort_lds's wave-rank pass over 128 chunks -- are 2048x8192-key_0 / -last_key.)"""
    from hassaku_amd import hip_ops
    assert _plan(n_keys, n)['kind'] == kind
    keys, want_perm, want_offsets = _keys(n_keys, n, dist)
    dkeys = torch.from_numpy(keys).cuda()
    if kind == 'unsupported':
        with pytest.raises(ValueError, match='too large for the item sort'):
            hip_ops.key_sort(dkeys, n_keys)
        return
    perm, offsets = (t.cpu().numpy() for t in hip_ops.key_sort(dkeys, n_keys))
    assert perm.dtype == np.int32 and offsets.dtype == np.int32
    assert np.array_equal(offsets, want_offsets)
    assert np.array_equal(perm, want_perm)
    if n_keys in TOUCHED_UNSUPPORTED:
        with pytest.raises(ValueError, match='too large for the item sort with a touched list'):
            hip_ops.key_sort(dkeys, n_keys, touched=True)
        return
    perm, offsets, touched, n_touched = (t.cpu().numpy() for t in hip_ops.key_sort(dkeys, n_keys, touched=True))
    assert np.array_equal(offsets, want_offsets)
    assert np.array_equal(perm, want_perm)
    assert np.array_equal(np.sort(touched[:int(n_touched[0])]), np.unique(keys))


@pytest.mark.gpu
def test_a_lazy_items_state_beyond_the_touched_list_limit_is_refused_up_front():
    """hsk_check_state (here through hsk_bprmf_init_workspace): with lazy_items the item sort keeps a touched list, so a
    state of 2 097 153 items is refused when it is made, under the limit that applies -- not at its first step of more
    than 8192 entries.  The same tables without lazy_items, and 2 097 152 items with it, are accepted."""
    from hassaku_amd import hip_ops

    def state(n_items, lazy_items):
        user_emb = torch.zeros(4, 2, device='cuda')
        item_emb = torch.zeros(n_items, 2, device='cuda')
        return hip_ops.BprMfFusedState(user_emb, item_emb, lr=1e-3, wd=0.0, max_batch=8, max_cols=2, lazy_users=False,
                                       lazy_items=lazy_items, overlap=False)

    assert _plan(2097153, 16, True)['kind'] == 'unsupported' and _plan(2097153, 16, False)['kind'] != 'unsupported'
    with pytest.raises(RuntimeError, match=r'n_items 2097153 too large for the item sort \(max 2097152 per device '
                                           r'with lazy_items\)'):
        state(2097153, True)
    assert state(2097153, False).st.lazy_items == 0
    assert state(2097152, True).st.lazy_items == 1


COUNT_CASES = [(2048, 8192, 'lds'), (500, 2048, 'small2'), (1000, 4096, 'small4'), (2047, 8192, 'small8'),
               (513, 9000, 'two_level')]


@pytest.mark.gpu
@pytest.mark.parametrize('n_keys, n, kind', COUNT_CASES, ids=[f'{c[0]}x{c[1]}' for c in COUNT_CASES])
def test_device_side_entry_count(n_keys, n, kind):
    """The entry count read from device memory (the sharded step's n_dev): the stable sort of the first n_valid entries,
    whatever valid keys lie behind them; offsets[n_keys] == n_valid.  n_valid = n - 1 takes k_sort_small through its
    padding branch on a full buffer, n_valid = n through the closing branch."""
    from hassaku_amd import hip_ops
    assert _plan(n_keys, n, True)['kind'] == kind
    keys = _keys(n_keys, n, 'uniform')[0]
    dkeys = torch.from_numpy(keys).cuda()
    for n_valid in (0, 1, n - 1, n):
        head = keys[:n_valid]
        tail = keys[n_valid:]                       # valid keys too: counted, they would show in every offset behind them
        assert tail.size == n - n_valid and np.all((tail >= 0) & (tail < n_keys))
        want_perm, want_offsets = _stable_index(head, n_keys)
        count = torch.tensor([n_valid], dtype=torch.int32, device='cuda')
        perm, offsets, touched, n_touched = (t.cpu().numpy() for t in hip_ops.key_sort(dkeys, n_keys, True, count))
        assert offsets[n_keys] == n_valid
        assert np.array_equal(offsets, want_offsets), n_valid
        assert np.array_equal(perm[:n_valid], want_perm), n_valid
        assert np.array_equal(np.sort(touched[:int(n_touched[0])]), np.unique(head)), n_valid
        perm, offsets = (t.cpu().numpy() for t in hip_ops.key_sort(dkeys, n_keys, n_valid=n_valid))
        assert np.array_equal(offsets, want_offsets) and np.array_equal(perm[:n_valid], want_perm), n_valid


@pytest.mark.gpu
@pytest.mark.parametrize('n_keys, n, kind, dims', EMB_CASES, ids=[f'{c[0]}x{c[1]}' for c in EMB_CASES])
def test_embedding_backward_adds_in_ascending_position(n_keys, n, kind, dims):
    """hsk_embedding_backward, bit for bit: each table row's gradient is the fp32 sum of its positions' rows added one at
    a time in ascending position, starting from zero; rows nobody named are +0."""
    from hassaku_amd import hip_ops
    keys = _emb_keys(n_keys, n)
    idx = torch.from_numpy(keys).cuda()
    for dim in dims:
        g = _payload(n, dim, dim + n)
        table = torch.zeros(n_keys, dim, device='cuda', requires_grad=True)
        status = hip_ops.new_status('cuda')
        hip_ops.embedding(table, idx, status).backward(torch.from_numpy(g).cuda())
        hip_ops.raise_on_status(status)
        got, want = table.grad.cpu().numpy(), _sequential_sums(keys, n_keys, g)
        assert np.array_equal(_bits(got), _bits(want)), (dim, int((_bits(got) != _bits(want)).any(1).sum()), 'rows differ')
        unnamed = np.bincount(keys, minlength=n_keys) == 0
        assert not _bits(got)[unnamed].any()


@pytest.mark.gpu
@pytest.mark.parametrize('reps, kind', CSR_REPS, ids=[kind for _, kind in CSR_REPS])
def test_sparse_rows_sum_backward_adds_in_ascending_position(reps, kind):
    """hsk_sparse_rows_sum_backward, bit for bit, with the batch's pair count in each sort's range: grad_Wt[c] is the
    fp32 sum of g[j] over the batch positions j whose row holds c, one at a time in ascending j from zero."""
    from hassaku_amd import hip_ops
    indptr, indices, _ = _hand_csr()
    csr = (torch.from_numpy(indptr).cuda(), torch.from_numpy(indices).cuda())
    idx, cols, pos = _csr_batch(reps)
    assert _plan(N_IN, len(cols))['kind'] == kind
    for dim in CSR_DIMS:
        g = _payload(len(idx), dim, dim + reps)
        Wt = torch.zeros(N_IN, dim, device='cuda', requires_grad=True)
        status = hip_ops.new_status('cuda')
        hip_ops.sparse_rows_sum(Wt, csr, torch.from_numpy(idx).cuda(), status).backward(torch.from_numpy(g).cuda())
        hip_ops.raise_on_status(status)
        got, want = Wt.grad.cpu().numpy(), _sequential_sums(cols, N_IN, g[pos])
        assert np.array_equal(_bits(got), _bits(want)), (dim, int((_bits(got) != _bits(want)).any(1).sum()), 'rows differ')
        unnamed = np.bincount(cols, minlength=N_IN) == 0
        assert unnamed.any() and not _bits(got)[unnamed].any()
