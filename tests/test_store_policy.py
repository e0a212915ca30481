"""The large-batch step at the row shapes where a store policy changes the store's form, held to the CPU oracle.

Rows that leave a kernel for good (item p/m/v, the owners' user p/m/v, partial gradient rows, ucur / mcur / vcur, the rows
brought up to date ahead of time) may leave with write-through stores (csrc/hsk_common.h: hsk_stg_wt, HSK_WT_STREAMS):
16 bytes per lane through a buffer descriptor built per row, the row's bytes as its bound.  What can go wrong there is
the addressing -- the bound, the lanes beyond a partial last chunk or slice, the fall-back for rows of fewer than four
floats per lane -- and the hand-off of rows between the two launches of a step (ucur / mcur / vcur).  Whatever mask the
library was built with, each shape below takes 6 steps the way bench.py issues them (hint_after_run + steps_sampled, in
three runs) on the batches the recorder drew, then flush(), and is compared with oracle.MfOracleTrainer: the loss of each
step, the tables by assert_adam_param_close, the moments to 1e-5 (helpers and tolerances of
test_step_paths_vs_oracle.py).  Each shape runs with lazy and with dense user AdamW.

  d320        V = 4, a partial last chunk (NCH = 2) and a partial last 256-float slice
  d320-wide   the same rows with more than 64 K entries: the D-sliced item pass instead of the whole-row one
  d402        V = 2: plain stores whatever the mask
  d65         V = 1
  p2-dups     P = 2, U << B: every user several times in a batch, owners publish through ucur / mcur / vcur
  p4-d2048    P = 4, NCH = 8: eight chunks' offsets under one descriptor
"""
import numpy as np
import pytest

import test_step_paths_vs_oracle as paths

pytestmark = pytest.mark.gpu

# users, items, D, B, N, expected P (hsk_part_rule)
SHAPES = {
    'wt-d320':      dict(U=700, I=900, D=320, B=2048, N=9, P=1),
    'wt-d320-wide': dict(U=700, I=900, D=320, B=2048, N=40, P=1),   # 2048 x 41 entries > 64 K
    'wt-d402':      dict(U=700, I=900, D=402, B=2048, N=9, P=1),
    'wt-d65':       dict(U=700, I=900, D=65, B=2048, N=9, P=1),
    'wt-p2-dups':   dict(U=300, I=8000, D=256, B=2048, N=17, P=2),
    'wt-p4-d2048':  dict(U=1000, I=2000, D=2048, B=2048, N=33, P=4),
}
STEPS = 6
for _name, _sc in SHAPES.items():
    paths.SCENARIOS[_name] = dict(_sc, steps=STEPS, loss='bpr', opt='adamw')
CASES = [(name, lazy) for name in SHAPES for lazy in (True, False)]


@pytest.fixture(scope='module')
def ops():
    from hassaku_amd import hip_ops
    return hip_ops


def _run(ops, d, lazy):
    """-> (snapshot, per-step losses).  Three runs of two steps; a run leaves the loss of its last step and the sum over
    the run (both fp64), so the first step's is their difference."""
    sc, order = d['sc'], d['dev']['order']
    B, N, sched = sc['B'], sc['N'], sc['schedule']
    st, t = paths._new_state(ops, d, lazy)
    losses, total = [], 0.0
    for first, m in paths._runs_of(sched):
        assert m == 2
        st.hint_after_run(order, sched[first][0] + m * B, B, N, n_batches=2)
        st.steps_sampled(order, sched[first][0], m, B, N)
        last, both = st.last_loss(), st.pop_loss_sum()
        losses += [both - last, last]
        total += both
    snap = paths._snapshot(st, t, d)
    snap['loss_sum'] = total      # _snapshot popped an empty sum
    return snap, losses


@pytest.mark.parametrize('name,lazy', CASES, ids=[f'{n[3:]}-{"lazy" if lz else "dense"}' for n, lz in CASES])
def test_large_batch_step_vs_oracle(ops, oracle, name, lazy):
    d = paths._data(ops, name)
    ref = paths._reference(ops, oracle, d, lazy)
    got, losses = _run(ops, d, lazy)
    if name == 'wt-p2-dups':
        u = ref['batches'][0][0]
        assert np.bincount(u).max() > 1 + 8, 'users beyond the owners\' duplicate lists'
    paths._hold_to_oracle(f'{name}-{"lazy" if lazy else "dense"}', got, ref, STEPS if SHAPES[name]['P'] > 1 else 0, 0,
                          step_losses=losses)
