"""The pair form of the item pass with its lists written out once per step (csrc/hsk_item_sliced.h: k_item_lists and
hsk_item_pair_body<PART, LISTS = true>) against the same form gathering its weights through the sort's permutation.

k_item_lists writes, for every sorted position c, the weight hsk_entry_weight<PART> gives entry perm[c] (for a positive
the P shares, added in the same order) and its batch position; the item waves then read both with two coalesced loads
per chunk of 64 entries.  The multiply-adds, their operands and their order are those of LISTS = false, so the claim is
bit-identity: two states on the same tables and batches, both with the pair form forced on (st.item_pair = 1; the rule
takes it only from B = 4096), one with st.item_lists = 1, one with -1, take 3 steps and flush(); user_emb, item_emb,
item_bias, every moment and the list of losses must be torch.equal.  The forced-on run is then held to
oracle.MfOracleTrainer with the bounds test_store_policy.py uses for large-batch steps (loss 1e-6 relative per step,
moments 1e-5 of the tensor's largest, tables by assert_adam_param_close).

Cases: the eight shapes of test_item_pair.py (sampled batches: P = 2 with BPR, BCE and dense users; D = 256, 192, 128,
1024; the 40 000-item catalogue with lists of 1-3 entries and one beyond 128), and `lengths`, hand-built batches through
step(u_idx, i_idx) at B = 2048 (the partitioned forward does not run below), D = 512, P = 2, in which chosen items have
lists of exactly 0, 1, 7, 8, 9, 63, 64, 65, 128 and 129 entries: both chunk boundaries (64, 128) and the boundary of a
full group of loads (2 x HSK_ITEM_PAIR_MLP = 8 entries).  For every length from 7 there are three such items, whose
positive's entry (the one that carries P shares) sits first, in the middle and last in the list -- the sort is stable,
so the place follows from the batch rows -- and one without a positive; one user is in the batch twice, and the table's
last rows (item I - 1 as a positive and as negatives, user U - 1) are named.  All of that is asserted on the batches and
on the device's own sort (last_sort)."""
import numpy as np
import pytest
import torch

from conftest import assert_adam_param_close, max_norm_err
from test_hip_parity import _fused_state, dev
import test_item_pair as pairs
import test_step_paths_vs_oracle as paths

pytestmark = pytest.mark.gpu

STEPS = 3
U, I, D, B, N, P_EXPECTED = 700, 3000, 512, 2048, 32, 2
LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 128, 129)
PLACES = ('first', 'middle', 'last', 'none')


@pytest.fixture(scope='module')
def ops():
    from hassaku_amd import hip_ops
    return hip_ops


def _specials():
    """[(item, length, place of the positive's entry)]; item I - 1 is the 9-entry list with the positive in the middle"""
    out, item = [], 40
    for L in LENGTHS:
        for place in PLACES:
            if (L == 0 and place != 'none') or (L == 1 and place in ('middle', 'last')):
                continue
            out.append((I - 1 if (L, place) == (9, 'middle') else item, L, place))
            item += 53
    return out


def _batch(rng, specials):
    """(u [B], i [B, 1 + N]): every special item in exactly `length` entries, everything else drawn from the other items"""
    special_items = np.array([s[0] for s in specials])
    others = np.setdiff1d(np.arange(I), special_items)
    i = others[rng.randint(0, len(others), size=(B, N + 1))].astype(np.int64)
    used = np.zeros((B, N + 1), dtype=bool)
    pos_rows = iter(rng.permutation(np.arange(200, B - 200)))   # rows with room in front of and behind them
    for item, L, place in specials:
        if L == 0:
            continue
        n_neg = L - (place != 'none')
        rp = int(next(pos_rows))
        if place == 'first':
            rows = rng.randint(rp + 1, B, size=n_neg)
        elif place == 'last':
            rows = rng.randint(0, rp, size=n_neg)
        elif place == 'middle':
            rows = np.concatenate([rng.randint(0, rp, size=n_neg // 2), rng.randint(rp + 1, B, size=n_neg - n_neg // 2)])
        else:
            rows = rng.randint(0, B, size=n_neg)
        if place != 'none':
            assert not used[rp, 0]
            i[rp, 0], used[rp, 0] = item, True
        for r in rows:
            free = np.flatnonzero(~used[r, 1:]) + 1
            c = int(free[rng.randint(len(free))])
            i[r, c], used[r, c] = item, True
    u = rng.randint(0, U, size=B).astype(np.int64)
    u[1] = u[0]          # one user twice
    u[5] = U - 1         # the user table's last row
    return u, i


_DATA = {}


def _data():
    """tables and batches of the `lengths` case, with what the docstring claims asserted on the batches"""
    if _DATA:
        return _DATA
    rng = np.random.RandomState(20)
    specials = _specials()
    params = {'user_emb': (rng.randn(U, D) * 0.05).astype(np.float32), 'item_emb': (rng.randn(I, D) * 0.05).astype(np.float32),
              'item_bias': (rng.randn(I) * 0.1).astype(np.float32)}
    batches = [_batch(rng, specials) for _ in range(STEPS)]
    assert {L for _, L, _ in specials} == set(LENGTHS)
    for L in LENGTHS:
        if L >= 7:
            assert {p for _, l, p in specials if l == L} == set(PLACES), L
    for u, i in batches:
        counts = np.bincount(i.reshape(-1), minlength=I)
        for item, L, place in specials:
            assert counts[item] == L, (item, L, counts[item])
            assert (i[:, 0] == item).sum() == (L > 0 and place != 'none'), (item, place)
        assert u[0] == u[1] and (u == U - 1).any()
        assert (i[:, 0] == I - 1).sum() == 1 and (i[:, 1:] == I - 1).sum() == 8, 'the item table\'s last row'
    _DATA.update(params=params, batches=batches, specials=specials)
    return _DATA


def _check_sort(st, specials):
    """the device's own lists of the last batch: the lengths, and where the positive's entry stands in each"""
    K = st.batch_columns(B, N + 1)
    assert K == N + P_EXPECTED, ('partitions', K)
    perm, offs = st.last_sort(B * K)
    perm, offs = perm.cpu().numpy(), offs.cpu().numpy()
    for item, L, place in specials:
        lst = perm[offs[item]:offs[item + 1]]
        assert len(lst) == L, (item, L, len(lst))
        is_pos = (lst % K == 0)
        assert is_pos.sum() == (L > 0 and place != 'none'), (item, place)
        if place == 'first':
            assert is_pos[0]
        elif place == 'last':
            assert is_pos[-1]
        elif place == 'middle':
            assert not is_pos[0] and not is_pos[-1]


def _run_lengths(ops, lists):
    d = _data()
    st, t = _fused_state(ops, d['params'], 1e-3, 1e-4, B, N + 1, loss='bpr', lazy_users=True)
    st.st.item_pair, st.st.item_lists = 1, lists
    losses = []
    for u, i in d['batches']:
        st.step(dev(u), dev(i))
        losses.append(st.last_loss())
    _check_sort(st, d['specials'])
    st.flush()
    st.check_status()
    return st, t, losses


def _same_bits(name, st_on, t_on, losses_on, st_off, t_off, losses_off):
    both = {k: (t_on[k], t_off[k]) for k in t_on}
    both.update({'m_' + k: (st_on.m[k], st_off.m[k]) for k in t_on})
    both.update({'v_' + k: (st_on.v[k], st_off.v[k]) for k in t_on})
    figs = {k: int((a != b).sum().item()) for k, (a, b) in both.items()}
    print(f'ROW {name}: elements that differ with and without the written lists {figs}; losses {losses_on} {losses_off}',
          flush=True)
    for k, (a, b) in both.items():
        assert torch.equal(a, b), (name, k, figs[k])
    assert losses_on == losses_off, (name, losses_on, losses_off)


def test_written_lists_same_bits_and_oracle_at_every_length(ops, oracle):
    d = _data()
    st_on, t_on, losses_on = _run_lengths(ops, 1)
    st_off, t_off, losses_off = _run_lengths(ops, -1)
    _same_bits('lengths', st_on, t_on, losses_on, st_off, t_off, losses_off)

    tr = oracle.MfOracleTrainer(d['params']['user_emb'], d['params']['item_emb'], d['params']['item_bias'], lr=1e-3, wd=1e-4,
                                loss='bpr')
    ref_losses = [tr.step(u, i)[0] for u, i in d['batches']]
    fig = {k: (max_norm_err(st_on.m[k].cpu().numpy().reshape(-1), tr.M[k].reshape(-1)),
               max_norm_err(st_on.v[k].cpu().numpy().reshape(-1), tr.V[k].reshape(-1))) for k in t_on}
    print('ROW lengths against the oracle: losses ' + ' '.join(f'{abs(a - b) / abs(b):.2e}' for a, b in zip(losses_on, ref_losses))
          + ' ' + ' '.join(f'{k}: m {a:.2e} v {b:.2e}' for k, (a, b) in fig.items()), flush=True)
    for s, (a, b) in enumerate(zip(losses_on, ref_losses)):
        assert abs(a - b) <= 1e-6 * abs(b), ('loss of step', s, a, b)
    for k in t_on:
        assert fig[k][0] < 1e-5, ('exp_avg', k, fig[k][0])
        assert fig[k][1] < 1e-5, ('exp_avg_sq', k, fig[k][1])
    for k in t_on:
        assert_adam_param_close(t_on[k].cpu().numpy(), tr.P[k], ('lengths', k))


def _run_sampled(ops, d, lazy, lists):
    """test_item_pair._run with the pair form on and the written lists forced on (1) or off (-1)"""
    sc, order = d['sc'], d['dev']['order']
    st, t = paths._new_state(ops, d, lazy)
    st.st.item_pair, st.st.item_lists = 1, lists
    losses = []
    for start, nb in sc['schedule']:
        st.step_sampled(order, start, nb, sc['N'])
        losses.append(st.last_loss())
    snap = paths._snapshot(st, t, d)   # (flushes)
    return st, t, losses, snap


@pytest.mark.parametrize('name', list(pairs.SHAPES), ids=[n[5:] for n in pairs.SHAPES])
def test_written_lists_same_bits_and_oracle(ops, oracle, name):
    lazy = pairs.SHAPES[name]['lazy']
    d = pairs._data(ops, name)
    st_on, t_on, losses_on, snap_on = _run_sampled(ops, d, lazy, 1)
    st_off, t_off, losses_off, _ = _run_sampled(ops, d, lazy, -1)
    _same_bits(name, st_on, t_on, losses_on, st_off, t_off, losses_off)
    ref = paths._reference(ops, oracle, d, lazy)
    paths._hold_to_oracle(name + '-lists', snap_on, ref, 0, 0, step_losses=losses_on)
