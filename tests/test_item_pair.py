"""The pair form of the large-batch item pass (csrc/hsk_item_sliced.h: hsk_item_pair_body) against the form it replaces.

The pair form cuts D into 128-float slices and loads two consecutive entries of an item's list with one instruction (the
two halves of a wave), then swaps registers between the halves so that every lane holds the same two floats of both
entries.  Each element still sees the same fmaf chain in list order, so the claim is bit-identity: two states built from
the same tables, seed and interactions, one with the form forced on (st.item_pair = 1), one with it forced off (-1), take
3 steps and flush(); user_emb, item_emb, item_bias, both item moments and the list of losses must be torch.equal.  That
also checks the lane pattern of v_permlane32_swap_b32 on the device: any other pattern moves floats between elements.
The forced-on run is then held to oracle.MfOracleTrainer by test_step_paths_vs_oracle._hold_to_oracle, with the
tolerances test_store_policy.py uses.

The sliced kernels run above 65 536 entries: B x (N + 1) = 2048 x 33.  Shapes (hsk_part_rule gives the P stated):

  d512-part   P = 2: the partitioned forward, so PART with the shares of the positive's weight; four slices
  d256        no partitions, two slices; ~113 entries per item: chunks of 64 plus a remainder, odd and even tails
  d192        the last slice half empty: `live` false in the upper lanes of each half-wave
  d128        one slice (n_slices_pad = 1)
  d1024       eight slices, one XCD each
  d256-hot    40 000 items: most lists have 0, 1, 2 or 3 entries; item 7 is the only positive of 130 users that are in
              every batch, so its list exceeds 128 entries
  d512-bce    d512-part with the BCE loss
  d512-dense  d512-part with dense user AdamW
"""
import numpy as np
import pytest
import torch

from conftest import csr_from_pairs
from test_hip_parity import dev
import test_step_paths_vs_oracle as paths

pytestmark = pytest.mark.gpu

STEPS = 3
HOT_ITEM, HOT_USERS = 7, 130
# users, items, D, B, N, expected P (hsk_part_rule), loss, lazy user AdamW
SHAPES = {
    'pair-d512-part':  dict(U=700, I=3000, D=512, B=2048, N=32, P=2, loss='bpr', lazy=True),
    'pair-d256':       dict(U=700, I=600, D=256, B=2048, N=32, P=1, loss='bpr', lazy=True),
    'pair-d192':       dict(U=700, I=600, D=192, B=2048, N=32, P=1, loss='bpr', lazy=True),
    'pair-d128':       dict(U=700, I=600, D=128, B=2048, N=32, P=1, loss='bpr', lazy=True),
    'pair-d1024':      dict(U=700, I=2000, D=1024, B=2048, N=32, P=2, loss='bpr', lazy=True),
    'pair-d256-hot':   dict(U=900, I=40000, D=256, B=2048, N=32, P=4, loss='bpr', lazy=True, hot=True),
    'pair-d512-bce':   dict(U=700, I=3000, D=512, B=2048, N=32, P=2, loss='bce', lazy=True),
    'pair-d512-dense': dict(U=700, I=3000, D=512, B=2048, N=32, P=2, loss='bpr', lazy=False),
}

@pytest.fixture(scope='module')
def ops():
    from hassaku_amd import hip_ops
    return hip_ops


_DATA = {}


def _data(ops, name):
    """The dictionary test_step_paths_vs_oracle._data builds for its own scenarios, for a shape of this file (the last
    one built is kept).  hot: HOT_USERS users have HOT_ITEM as their only positive, and the interaction order puts
    those users into every batch."""
    if name in _DATA:
        return _DATA[name]
    _DATA.clear()
    sc = dict({k: v for k, v in SHAPES[name].items() if k not in ('lazy', 'hot')}, steps=STEPS, opt='adamw', lr=1e-3,
              wd=1e-4, name=name)
    sc['schedule'] = paths._schedule(sc)
    U, I, D, B = sc['U'], sc['I'], sc['D'], sc['B']
    rng = np.random.RandomState(sum(map(ord, name)))
    n_batches = sc['steps'] + 2                                   # two batches behind the last run may be named
    if SHAPES[name].get('hot'):
        rest = paths._skewed_pairs(rng, U - HOT_USERS, I)
        rest = rest[rest[:, 1] != HOT_ITEM]
        rest[:, 0] += HOT_USERS
        hot = np.stack([np.arange(HOT_USERS, dtype=np.int64), np.full(HOT_USERS, HOT_ITEM, dtype=np.int64)], axis=1)
        pairs = np.concatenate([hot, rest])
        order = np.concatenate([rng.permutation(np.concatenate([np.arange(HOT_USERS), HOT_USERS + rng.choice(
            len(rest), B - HOT_USERS, replace=False)])) for _ in range(n_batches)]).astype(np.int64)
    else:
        pairs = paths._skewed_pairs(rng, U, I)
        reps = -(-n_batches * B // len(pairs))
        order = np.concatenate([np.random.RandomState(6 + r).permutation(len(pairs)) for r in range(reps)])
    ptr, idx = csr_from_pairs(pairs, U)
    P = {'user_emb': (rng.randn(U, D) * 0.05).astype(np.float32), 'item_emb': (rng.randn(I, D) * 0.05).astype(np.float32),
         'item_bias': (rng.randn(I) * 0.1).astype(np.float32)}
    _DATA[name] = dict(sc=sc, pairs=pairs, ptr=ptr, idx=idx, P=P, order=order, alias=None,
                       dev=dict(ptr=dev(ptr), idx=dev(idx), cu=dev(pairs[:, 0], torch.int32),
                                ci=dev(pairs[:, 1], torch.int32), order=torch.from_numpy(order).cuda(), alias=None))
    return _DATA[name]


def _run(ops, d, lazy, pair):
    """3 x step_sampled with the form forced on (1) or off (-1), flush -> (snapshot, losses, list lengths of the last
    batch, item moments and tables as device tensors)"""
    sc, order = d['sc'], d['dev']['order']
    st, t = paths._new_state(ops, d, lazy)
    st.st.item_pair = pair
    losses = []
    for start, nb in sc['schedule']:
        st.step_sampled(order, start, nb, sc['N'])
        losses.append(st.last_loss())
    B, K = sc['B'], sc['N'] + 1
    _, bi = st.last_batch(B, K)
    _, offs = st.last_sort(B * st.batch_columns(B, K))
    lengths = np.diff(offs.cpu().numpy())
    assert np.array_equal(lengths, np.bincount(bi.cpu().numpy().reshape(-1), minlength=sc['I'])), 'the sort\'s lists'
    snap = paths._snapshot(st, t, d)
    tensors = dict(user_emb=t['user_emb'], item_emb=t['item_emb'], item_bias=t['item_bias'],
                   m_item_emb=st.m['item_emb'], v_item_emb=st.v['item_emb'])
    return snap, losses, lengths, tensors


@pytest.mark.parametrize('name', list(SHAPES), ids=[n[5:] for n in SHAPES])
def test_pair_form_same_bits_and_oracle(ops, oracle, name):
    lazy = SHAPES[name]['lazy']
    d = _data(ops, name)
    on, losses_on, lengths, t_on = _run(ops, d, lazy, 1)
    off, losses_off, _, t_off = _run(ops, d, lazy, -1)
    figs = {k: int((t_on[k] != t_off[k]).sum().item()) for k in t_on}
    print(f'ROW {name}: elements that differ between the forms {figs}; losses {losses_on} {losses_off}; lists: '
          f'{int((lengths == 1).sum())} of length 1, {int(((lengths % 2 == 1) & (lengths > 1)).sum())} odd beyond 1, '
          f'{int((lengths > 64).sum())} beyond 64, longest {int(lengths.max())}', flush=True)
    for k in t_on:
        assert torch.equal(t_on[k], t_off[k]), (name, k, figs[k])
    assert losses_on == losses_off, (name, losses_on, losses_off)
    if SHAPES[name].get('hot'):
        # a list of one entry, an odd chunk tail, and more than one chunk of 64 -- here more than two
        assert (lengths == 1).any() and ((lengths % 2 == 1) & (lengths > 1)).any() and (lengths > 64).any(), name
        assert lengths[HOT_ITEM] > 128, lengths[HOT_ITEM]
    ref = paths._reference(ops, oracle, d, lazy)
    paths._hold_to_oracle(name, on, ref, 0, 0, step_losses=losses_on)
