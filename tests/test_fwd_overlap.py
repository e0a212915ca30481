"""The overlapped gather loop of the item-partitioned forward (csrc/hsk_fwd_part.h: k_fwd_part<..., OVL = true>) against
the loop it replaces.

The overlapped loop issues every load of a buffer on every path -- an entry beyond the end of a unit's list repeats
the chunk's last entry, or names the positive's row where the list is empty -- weighs full buffers without a test per row and peels the last, partial
buffers of a chunk.  Operands, fmaf chains, the lane tree and the order of the sums are those of the old loop, so the
claim is bit-identity: two states on the same tables and hand-built batches, one with st.fwd_overlap = 1, one with -1,
take 3 steps and flush(); user_emb, item_emb, item_bias, every moment and the list of losses must be torch.equal.  The
forced-on run is then held to oracle.MfOracleTrainer with the bounds test_store_policy.py uses for large-batch steps
(loss 1e-6 relative, moments 1e-5 of the tensor's largest, tables by assert_adam_param_close).

What the full / tail split distinguishes is the length of a (positive, partition) list against R, the rows of a buffer:
R = 3 at D = 256 and 512, R = 2 at D = 1024 (hsk_fused.hip: RP); R = 4 is covered as well.  The batches go through
step(u_idx, i_idx) as in test_fwd_row_groups.py: the number of negatives of positive b in partition 0 (and 1, 2 at
P = 4) cycles through COUNTS, the last partition takes the complement to N.  Four consecutive positives are the four
waves of one workgroup, so a workgroup mixes the lengths.  COUNTS holds 0, 1, R - 1, R, R + 1, 2R - 1, 2R, 2R + 1, 3R,
4R - 1, 4R, 4R + 1 for R = 2, 3, 4, the chunk boundaries 62-67 and 126-130 -- asserted on the batches themselves.

Address safety of the always-issued loads is a matter of the index arithmetic (the lane index is clamped to the chunk's
last entry, max(nr, 1) - 1 <= 63; lanes at and beyond the list's end hold the positive's id, so lane 0 of an empty list
does), read there and not provoked here; the cases below only make sure
the values those loads bring are never used: lists of exactly 64 and 65 entries (the last entry in lane 63, a second
chunk of one entry in lane 0), empty lists, positives and negatives that are the table's last row.

The partitioned forward runs from B = 2048 (hsk_part_rule), so that is the batch of every case."""
import numpy as np
import pytest
import torch

from conftest import assert_adam_param_close, max_norm_err
from test_hip_parity import _fused_state, dev

pytestmark = pytest.mark.gpu

STEPS = 3
N_NEG = 136
B = 2048
COUNTS = (list(range(0, 10)) + [11, 12, 13, 15, 16, 17] + list(range(62, 68)) + list(range(126, 131)))
LENGTHS = set(COUNTS)

# name: users, items, D, expected P (hsk_part_rule), loss, lazy user AdamW
CASES = {
    'p4-d512-bpr-lazy':  (1500, 10677, 512, 4, 'bpr', True),     # the headline instantiation, R = 3
    'p4-d512-bce-dense': (1500, 10677, 512, 4, 'bce', False),
    'p2-d256-bpr-dense': (700, 8000, 256, 2, 'bpr', False),      # one chunk per row, R = 3
    'p2-d256-bce-lazy':  (700, 8000, 256, 2, 'bce', True),
    'p2-d1024-bpr-lazy': (700, 2000, 1024, 2, 'bpr', True),      # R = 2
}


@pytest.fixture(scope='module')
def ops():
    from hassaku_amd import hip_ops
    return hip_ops


def _bounds(n_items, n_part):
    """partition q = items [ceil(q I / P), ceil((q + 1) I / P))"""
    return [-(-q * n_items // n_part) for q in range(n_part + 1)]


def _batch(rng, step, U, I, n_part):
    """(u [B], i [B, 1 + N], counts [B, P]).  The columns of a row are shuffled, so a unit's list is picked out of every
    64-column group.  Every fifth positive is the table's last row; in every third row the last partition's first
    negative is the table's last row."""
    u = rng.randint(0, U, size=B).astype(np.int64)
    i = np.empty((B, N_NEG + 1), dtype=np.int64)
    i[:, 0] = rng.randint(0, I, size=B)
    i[::5, 0] = I - 1
    bnd = _bounds(I, n_part)
    cnt = np.zeros((B, n_part), dtype=np.int64)
    nc = len(COUNTS)
    for b in range(B):
        left = N_NEG
        cnt[b, 0] = min(left, COUNTS[(b + step) % nc])
        left -= cnt[b, 0]
        for q, (mul, add) in zip(range(1, n_part - 1), ((7, 3), (11, 5))):
            cnt[b, q] = min(left, COUNTS[(b * mul + add + step) % nc])
            left -= cnt[b, q]
        cnt[b, n_part - 1] = left
        neg = [rng.randint(bnd[q], bnd[q + 1], size=cnt[b, q]) for q in range(n_part)]
        if b % 3 == 0 and cnt[b, n_part - 1] > 0:
            neg[n_part - 1][0] = I - 1
        i[b, 1:] = np.concatenate(neg)[rng.permutation(N_NEG)]
    return u, i, cnt


_DATA = {}


def _data(name):
    """tables and batches of a case (the last one built is kept), with the properties the docstring claims asserted"""
    if name in _DATA:
        return _DATA[name]
    _DATA.clear()
    U, I, D, P, loss, lazy = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    params = {'user_emb': (rng.randn(U, D) * 0.05).astype(np.float32), 'item_emb': (rng.randn(I, D) * 0.05).astype(np.float32),
              'item_bias': (rng.randn(I) * 0.1).astype(np.float32)}
    batches = [_batch(rng, s, U, I, P) for s in range(STEPS)]
    bnd = _bounds(I, P)
    for u, i, cnt in batches:   # the counts are what the kernel's partition test will find
        for q in range(P):
            assert np.array_equal(((i[:, 1:] >= bnd[q]) & (i[:, 1:] < bnd[q + 1])).sum(axis=1), cnt[:, q])
        assert (i[:, 0] == I - 1).any() and (i[:, 1:] == I - 1).any(), 'the table\'s last row'
        for q in range(P):      # every unit column sees the lengths mixed inside a workgroup (4 consecutive positives)
            groups = cnt[:, q].reshape(-1, 4)
            assert (np.array([len(set(g)) for g in groups]) >= 3).mean() > 0.5, q
    seen = set(np.unique(np.concatenate([cnt.reshape(-1) for _, _, cnt in batches])).tolist())
    assert LENGTHS <= seen, sorted(LENGTHS - seen)
    _DATA[name] = dict(params=params, batches=batches)
    return _DATA[name]


def _run(ops, name, overlap):
    """3 steps with the overlapped loop forced on (1) or off (-1), flush -> (state, tables, per-step losses)"""
    U, I, D, P, loss, lazy = CASES[name]
    d = _data(name)
    st, t = _fused_state(ops, d['params'], 1e-3, 1e-4, B, N_NEG + 1, loss=loss, lazy_users=lazy)
    assert st.batch_columns(B, N_NEG + 1) == N_NEG + P, ('partitions', name)
    st.st.fwd_overlap = overlap
    losses = []
    for u, i, _ in d['batches']:
        st.step(dev(u), dev(i))
        losses.append(st.last_loss())
    st.flush()
    st.check_status()
    return st, t, losses


@pytest.mark.parametrize('name', list(CASES))
def test_overlapped_loop_same_bits_and_oracle(ops, oracle, name):
    U, I, D, P, loss, lazy = CASES[name]
    d = _data(name)
    st_on, t_on, losses_on = _run(ops, name, 1)
    st_off, t_off, losses_off = _run(ops, name, -1)
    pairs = {k: (t_on[k], t_off[k]) for k in t_on}
    pairs.update({'m_' + k: (st_on.m[k], st_off.m[k]) for k in t_on})
    pairs.update({'v_' + k: (st_on.v[k], st_off.v[k]) for k in t_on})
    figs = {k: int((a != b).sum().item()) for k, (a, b) in pairs.items()}
    print(f'ROW {name}: elements that differ between the loops {figs}; losses {losses_on} {losses_off}', flush=True)
    for k, (a, b) in pairs.items():
        assert torch.equal(a, b), (name, k, figs[k])
    assert losses_on == losses_off, (name, losses_on, losses_off)

    tr = oracle.MfOracleTrainer(d['params']['user_emb'], d['params']['item_emb'], d['params']['item_bias'], lr=1e-3, wd=1e-4,
                                loss=loss)
    ref_losses = [tr.step(u, i)[0] for u, i, _ in d['batches']]
    fig = {k: (max_norm_err(st_on.m[k].cpu().numpy().reshape(-1), tr.M[k].reshape(-1)),
               max_norm_err(st_on.v[k].cpu().numpy().reshape(-1), tr.V[k].reshape(-1))) for k in t_on}
    print(f'ROW {name} against the oracle: losses ' + ' '.join(f'{abs(a - b) / abs(b):.2e}' for a, b in zip(losses_on, ref_losses))
          + ' ' + ' '.join(f'{k}: m {a:.2e} v {b:.2e}' for k, (a, b) in fig.items()), flush=True)
    for s, (a, b) in enumerate(zip(losses_on, ref_losses)):
        assert abs(a - b) <= 1e-6 * abs(b), (name, 'loss of step', s, a, b)
    for k in t_on:
        assert fig[k][0] < 1e-5, (name, 'exp_avg', k, fig[k][0])
        assert fig[k][1] < 1e-5, (name, 'exp_avg_sq', k, fig[k][1])
    for k in t_on:
        assert_adam_param_close(t_on[k].cpu().numpy(), tr.P[k], (name, k))
