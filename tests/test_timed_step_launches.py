"""The separate launches of a timed training step (csrc/hsk_fused.hip: `timed_apart`) against the merged launch and the oracle.

When the item or the user stage is timed, an even-D step does not run its usual single item + user launch: the item pass
goes out alone (k_item_update_sliced, or k_item_update_rows under lazy item AdamW) and k_user_update_lazy /
k_user_update_dense follow in a launch of their own -- the PART flavours of both where the forward was item-partitioned.
Only `bench.py --time-all-stages` asks for that; this file pins it.

Each case takes 3 steps through step(u_idx, i_idx) on seeded batches, then flush(): once with
enable_timing(('fwd', 'item', 'user'), every=1), once on an untimed twin state built from the same tables.
  * both runs are held to oracle.MfOracleTrainer with the bounds of test_fwd_overlap.py (loss 1e-6 relative, moments
    1e-5 of the tensor's largest, tables by assert_adam_param_close);
  * the timed run equals the twin bit for bit: tables, moments and losses (the separate kernels sum in the order of
    the merged one; measured before the launch layer was touched: 0 differing elements in every case);
  * collect_timing() reports `fwd` with exactly 3 samples and `user` with at least 3 (a periodic sweep records under
    `user` as well).  `item` has exactly 3, and exactly 6 under lazy item AdamW, whose catch-up launch in front of the
    forward is bracketed as `item` too.

Shapes: the smallest that reach each branch.  p2-d256 is partitioned (hsk_part_rule: a 7.8 MB table, n_neg >= 8 P gives
P = 2, asserted through batch_columns) and runs lazy and dense users under AdamW (GEN = false) and Adam (GEN = true);
small-d64 is the unpartitioned step, lazy and dense; small-d64-lazy-items takes k_item_update_rows, which otherwise only
the sharded step reaches."""
import numpy as np
import pytest
import torch

from conftest import assert_adam_param_close, max_norm_err
from test_hip_parity import _fused_state, dev

pytestmark = pytest.mark.gpu

STEPS = 3
LR, WD = 1e-3, 1e-4

# name: users, items, D, B, N, expected P (hsk_part_rule)
SHAPES = {
    'p2-d256':   (700, 8000, 256, 2048, 16, 2),
    'small-d64': (300, 200, 64, 48, 9, 1),
}
# name: shape, lazy user AdamW, optimizer, lazy item AdamW
CASES = {
    'p2-d256-lazy-adamw':    ('p2-d256', True, 'adamw', False),
    'p2-d256-dense-adamw':   ('p2-d256', False, 'adamw', False),
    'p2-d256-lazy-adam':     ('p2-d256', True, 'adam', False),
    'p2-d256-dense-adam':    ('p2-d256', False, 'adam', False),
    'small-d64-lazy':        ('small-d64', True, 'adamw', False),
    'small-d64-dense':       ('small-d64', False, 'adamw', False),
    'small-d64-lazy-items':  ('small-d64', True, 'adamw', True),
}


@pytest.fixture(scope='module')
def ops():
    from hassaku_amd import hip_ops
    return hip_ops


_DATA, _REF = {}, {}


def _data(shape):
    if shape not in _DATA:
        U, I, D, B, N, P = SHAPES[shape]
        rng = np.random.RandomState(sum(map(ord, shape)))
        params = {'user_emb': (rng.randn(U, D) * 0.05).astype(np.float32), 'item_emb': (rng.randn(I, D) * 0.05).astype(np.float32),
                  'item_bias': (rng.randn(I) * 0.1).astype(np.float32)}
        batches = [(rng.randint(0, U, size=B).astype(np.int64), rng.randint(0, I, size=(B, N + 1)).astype(np.int64))
                   for _ in range(STEPS)]
        _DATA[shape] = dict(params=params, batches=batches)
    return _DATA[shape]


def _reference(oracle, shape, opt):
    """the oracle's 3 steps, computed once per (shape, optimizer) and left unchanged: lazy and dense updates agree after a flush"""
    if (shape, opt) not in _REF:
        d = _data(shape)
        tr = oracle.MfOracleTrainer(d['params']['user_emb'], d['params']['item_emb'], d['params']['item_bias'], lr=LR, wd=WD,
                                    optimizer=opt)
        losses = [tr.step(u, i)[0] for u, i in d['batches']]
        _REF[(shape, opt)] = (tr, losses)
    return _REF[(shape, opt)]


def _run(ops, name, timed):
    shape, lazy, opt, lazy_items = CASES[name]
    U, I, D, B, N, P = SHAPES[shape]
    d = _data(shape)
    st, t = _fused_state(ops, d['params'], LR, WD, B, N + 1, lazy_users=lazy, optimizer=opt, lazy_items=lazy_items)
    assert st.batch_columns(B, N + 1) == N + P, ('partitions', name)
    if timed:
        st.enable_timing(('fwd', 'item', 'user'), every=1)
    losses = []
    for u, i in d['batches']:
        st.step(dev(u), dev(i))
        losses.append(st.last_loss())
    st.flush()
    st.check_status()
    return st, t, losses, (st.collect_timing() if timed else None)


def _hold_to_oracle(name, what, st, t, losses, tr, ref_losses):
    fig = {k: (max_norm_err(st.m[k].cpu().numpy().reshape(-1), tr.M[k].reshape(-1)),
               max_norm_err(st.v[k].cpu().numpy().reshape(-1), tr.V[k].reshape(-1))) for k in t}
    print(f'ROW {name} {what} against the oracle: losses ' + ' '.join(f'{abs(a - b) / abs(b):.2e}' for a, b in zip(losses, ref_losses))
          + ' ' + ' '.join(f'{k}: m {a:.2e} v {b:.2e}' for k, (a, b) in fig.items()), flush=True)
    for s, (a, b) in enumerate(zip(losses, ref_losses)):
        assert abs(a - b) <= 1e-6 * abs(b), (name, what, 'loss of step', s, a, b)
    for k in t:
        assert fig[k][0] < 1e-5, (name, what, 'exp_avg', k, fig[k][0])
        assert fig[k][1] < 1e-5, (name, what, 'exp_avg_sq', k, fig[k][1])
    for k in t:
        assert_adam_param_close(t[k].cpu().numpy(), tr.P[k], (name, what, k))


@pytest.mark.parametrize('name', list(CASES))
def test_timed_step_equals_untimed_step_and_oracle(ops, oracle, name):
    shape, lazy, opt, lazy_items = CASES[name]
    st_t, t_t, losses_t, timing = _run(ops, name, True)
    st_u, t_u, losses_u, _ = _run(ops, name, False)
    tr, ref_losses = _reference(oracle, shape, opt)

    pairs = {k: (t_t[k], t_u[k]) for k in t_t}
    pairs.update({'m_' + k: (st_t.m[k], st_u.m[k]) for k in t_t})
    pairs.update({'v_' + k: (st_t.v[k], st_u.v[k]) for k in t_t})
    figs = {k: int((a != b).sum().item()) for k, (a, b) in pairs.items()}
    print(f'ROW {name}: elements that differ between the timed and the untimed step {figs}; losses {losses_t} {losses_u}; '
          f'samples {({s: n for s, (_, n) in timing.items()})}', flush=True)

    _hold_to_oracle(name, 'timed', st_t, t_t, losses_t, tr, ref_losses)
    _hold_to_oracle(name, 'untimed', st_u, t_u, losses_u, tr, ref_losses)

    for k, (a, b) in pairs.items():
        assert torch.equal(a, b), (name, k, figs[k])
    assert losses_t == losses_u, (name, losses_t, losses_u)

    assert timing['fwd'][1] == STEPS, (name, timing)
    assert timing['item'][1] == (2 * STEPS if lazy_items else STEPS), (name, timing)
    assert timing['user'][1] >= STEPS, (name, timing)
