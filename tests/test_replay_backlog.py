"""The lazy optimiser replay over long backlogs and past the per-step scalar table.

A lazily updated row replays its pending zero-gradient steps in blocks of 64 per-step scalars, and beyond step
HSK_ADAM_TAB_LEN = 65 536 it reads the table's last entry.  The other lazy-vs-dense tests end every backlog at <= 64
steps (the sweep cadence of small batches) and stay far below the table's end.  Here hand-built schedules
(tests/replay_restate.py) put rows 0 .. 253 steps behind when they are touched and 260 behind at the closing sweep
(the two B = 2048 cases: the same list in 200 steps, the longest backlog 198 -- nothing >= 250 there),
with moments preloaded non-zero so that every replayed step's scalars show in the row, and runs start at a given step
(BprMfFusedState(start_step=...)) to cross the table's end.

Per case three runs: lazy, dense, oracle.  (1) lazy == dense, bit for bit, on every parameter, moment and loss -- the
project's claim; (2) dense is close to the oracle at the suite's bounds (loss 1e-6, moments 1e-5 of the tensor's largest,
parameters by assert_adam_param_close); (3) rows no batch touched follow the float64 zero-gradient chain within the
rounding bound derived in replay_restate (measured / bound is printed).

Which kernel a shape reaches is read from csrc/hsk_fused.hip (hsk_run_step): B <= 1024, bpr / bce, K >= 2 columns
-> k_fwd_ugrad_wg (8 waves at K >= 33 and B <= 256, else 4); sampled softmax or B > 1024 -> k_fwd_ugrad; the
partitioned forward where batch_columns() reports extra columns.  Lazy items on one device always take the whole-row
item pass (k_item_user_small -> hsk_item_row_body), the form whose `pend` loop these cases reach.

With the default betas the per-step scalars stop changing near t = 16 600, so the table's last entries are all equal;
one case takes a beta1 whose step_size settles exactly at t = 65 536 to hold the rule "beyond the table: its LAST entry".

Routing.  batch_columns(), key_sort_plan(), graph_replays() and pipelined_steps() are asserted where they tell the
path.  The library reports nothing about three paths: the hinted small-batch case (hsk_user_ahead_body in workgroups of
the item launch), the catchup_apart cases (k_user_catch_up) and the HSK_FLUSH_WAVE=0 child (k_user_flush).  That
those cases reach their kernels rests on reading hsk_run_step / hsk_launch_flush and on the mutation table in
MEASUREMENTS (a mutation inside each of the three kernels fails exactly these cases).

Not reached here: the sliced item pass's `pend` loop (behind HSK_ITEM_ROWS=0 / the sharded step), the sharded
catch-up (hsk_shard.inc; k_user_catch_up itself runs through catchup_apart).
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import replay_restate as R
from conftest import assert_adam_param_close, csr_from_pairs, max_norm_err

LR, WD = 2e-3, 1e-4
N_PROBES = len(R.LONG_PLAN)


# ---------------------------------------------------------------------------------------------------
# schedules (CPU)
# ---------------------------------------------------------------------------------------------------
PLANS = {'long': (R.LONG_PLAN, R.LONG_STEPS), 'short': (R.SHORT_PLAN, R.SHORT_STEPS), 'edge': (R.EDGE_PLAN, R.EDGE_STEPS)}
assert all(len(plan) == N_PROBES for plan, _ in PLANS.values())


def _plan(kind):
    return PLANS[kind]


def _row_schedule(n_rows, per_step, kind, n_busy, seed, replace=False, placed=None):
    """Probes are the last N_PROBES rows, the busy pool the first n_busy; the rows between are in no batch."""
    plan, n_steps = _plan(kind)
    probes = {n_rows - N_PROBES + k: steps for k, steps in enumerate(plan)}
    sched = R.schedule(n_rows, n_steps, per_step, probes, np.arange(n_busy), seed, replace=replace, placed=placed)
    sched['probes'] = sorted(probes)
    return sched


# the return batch of four probes holds the user 2, 9, 10 and 70 times: the ranked list (9 = exactly full), the batch
# scan, and a scan that runs through b = 64 from an owner that is not at the start of a chunk
DUP_PLACED = {
    (1, 68): [7, 50],                                        # probe 1 returns 64 behind, twice
    (2, 129): [3, 5, 6, 9, 20, 33, 64, 65, 95],              # 126 behind, 9 entries
    (5, 195): [66, 67, 70, 71, 72, 80, 81, 90, 93, 95],      # 192 behind, 10 entries, owner in the second chunk
    (8, 259): list(range(5, 75)),                            # 253 behind, 70 entries across b = 64
}

# name -> what the GPU cases below run; checked on the CPU for the backlogs they claim
SHAPES = {
    #               U     I     D    B    N  busy users
    'wg4':      (400,  200,  64,   96,   4, 200),
    'wg4_d402': (400,  200,  402,  96,   4, 200),
    'wg8':      (400,  200,  64,   8,   33, 100),
    'wg8_d402': (400,  200,  402,  8,   33, 100),
    'apart640': (400,  200,  640,  96,   4, 200),
    'items':    (300,  3000, 64,   48,   9, 150),
    'sweep33':  (400,  64,   33,   24,   3, 100),
    'sweep402': (400,  64,   402,  24,   3, 100),
    'sweep512': (400,  64,   512,  24,   3, 100),
    'sweep64':  (400,  64,   64,   24,   3, 100),
    'part':     (3000, 6000, 256,  2048, 16, 1000),
    'sampled':  (400,  300,  64,   64,   70, 150),
    'graph':    (400,  300,  64,   64,   9, 150),
}
ITEM_BUSY = 600


def _schedules(shape, kind, dups=False):
    U, I, D, B, N, busy = SHAPES[shape]
    placed = None
    if dups:
        placed = {(U - N_PROBES + k, s): pos for (k, s), pos in DUP_PLACED.items()}
    us = _row_schedule(U, B, kind, busy, seed=11, replace=B > busy, placed=placed)
    its = _row_schedule(I, B * (N + 1), kind, ITEM_BUSY, seed=12, replace=True) if shape == 'items' else None
    return us, its


EDGE_START = R.TAB_LEN - R.EDGE_AT

# the cases of the GPU tests below; the CPU tests assert the schedule of every (shape, plan) pair that occurs here
FORWARD_CASES = [   # shape, optimiser, loss, plan, start step
    ('wg4', 'adamw', 'bpr', 'long', 0), ('wg4_d402', 'adamw', 'bpr', 'long', 0),          # k_fwd_ugrad_wg<.., 4>
    ('wg8', 'adamw', 'bpr', 'long', 0), ('wg8_d402', 'adamw', 'bpr', 'long', 0),          # k_fwd_ugrad_wg<.., 8>
    ('wg4', 'adamw', 'sampled_softmax', 'long', 0), ('wg4_d402', 'adamw', 'sampled_softmax', 'long', 0),   # k_fwd_ugrad
    ('wg4', 'adam', 'bpr', 'long', 0), ('wg4', 'adagrad', 'bpr', 'long', 0),
    ('wg4', 'adamw', 'bpr', 'edge', EDGE_START), ('wg4', 'adam', 'bpr', 'edge', EDGE_START),
    ('wg4', 'adagrad', 'bpr', 'edge', EDGE_START), ('wg4', 'adamw', 'sampled_softmax', 'edge', EDGE_START),
    ('wg4', 'adamw', 'bpr', 'edge', 1_000_000),
]
PART_CASE = ('part', 'short', 0)
APART_CASES = [('wg4', 'adamw'), ('apart640', 'adamw'), ('wg4', 'adam')]                   # all on the long plan
ITEM_CASES = [('adamw', 'long', 0), ('adam', 'long', 0), ('adagrad', 'long', 0),
              ('adamw', 'edge', EDGE_START), ('adam', 'edge', EDGE_START)]
SWEEP_CASES = [
    ('sweep33', 'adamw', 'long', 0), ('sweep64', 'adamw', 'long', 0), ('sweep402', 'adamw', 'long', 0),
    ('sweep512', 'adamw', 'long', 0), ('sweep64', 'adam', 'long', 0), ('sweep64', 'adagrad', 'long', 0),
    ('sweep64', 'adamw', 'edge', EDGE_START), ('sweep402', 'adamw', 'edge', EDGE_START),
    ('sweep33', 'adagrad', 'edge', EDGE_START)]
SAMPLED_CASES = [('sampled', 'hinted', 'long', 0), ('graph', 'run', 'long', 0), ('graph', 'run', 'edge', EDGE_START),
                 ('part', 'run', 'short', 0)]
TABLE_END_CASE = ('wg4', 'edge')       # test_last_table_entry_is_the_one_used_beyond_the_table
FLUSH_CHILD_CASE = ('sweep64', 'long')
DUP_CASE = ('wg4', 'long')

GPU_SCHEDULES = sorted({(c[0], c[3]) for c in FORWARD_CASES} | {PART_CASE[:2]} | {(s, 'long') for s, _ in APART_CASES} |
                       {('items', k) for _, k, _ in ITEM_CASES} | {(c[0], c[2]) for c in SWEEP_CASES} |
                       {(c[0], c[2]) for c in SAMPLED_CASES} | {TABLE_END_CASE, FLUSH_CHILD_CASE, DUP_CASE})
assert {s for s, _ in GPU_SCHEDULES} == set(SHAPES)


@pytest.mark.parametrize('shape,kind', [c for c in GPU_SCHEDULES if c[1] in ('long', 'short')])
def test_schedules_hold_the_backlogs_they_claim(shape, kind):
    """Every backlog of REQUIRED_BACKLOGS at a touch of a probe; the long plan also two >= 250 (the short one, 200 steps
    for the B = 2048 cases, ends at 198); the rows outside every batch are behind by the whole run at the closing sweep."""
    n_steps = _plan(kind)[1]
    us, its = _schedules(shape, kind)
    for sched in (us, its):
        if sched is None:
            continue
        assert len(sched['batches']) == n_steps
        at_touch = {b for r in sched['probes'] for _, b in sched['backlogs'][r]}
        assert set(R.REQUIRED_BACKLOGS) <= at_touch, sorted(set(R.REQUIRED_BACKLOGS) - at_touch)
        if kind == 'long':
            assert sum(b >= 250 for b in at_touch) >= 2
        else:
            assert max(at_touch) == 198
        assert len(sched['untouched']) >= 20 and (sched['final'][sched['untouched']] == n_steps).all()
        assert not set(sched['untouched']) & set(sched['probes'])


@pytest.mark.parametrize('shape', [s for s, k in GPU_SCHEDULES if k == 'edge'])
def test_edge_schedules_lie_on_both_sides_of_the_table_end(shape):
    us, its = _schedules(shape, 'edge')
    for sched in (us, its):
        if sched is None:
            continue
        at_touch = {b for r in sched['probes'] for _, b in sched['backlogs'][r]}
        assert set(R.EDGE_BACKLOGS) <= at_touch, sorted(set(R.EDGE_BACKLOGS) - at_touch)
        below, across, above = R.crosses_edge(sched, sched['probes'])
        assert below >= 8 and across >= 8 and above >= 8, (below, across, above)
        # the 63 .. 66 and 127 .. 130 backlogs each have a 64-block that contains the table's end
        spanning = {b for r in sched['probes'] for s, b in sched['backlogs'][r] if s - b <= R.EDGE_AT <= s - 1}
        assert {64, 65, 127, 128, 129, 130} <= spanning, sorted(spanning)
        # ... and 62 .. 64 end just below / at it, 63 starts just above it
        ends = {(b, s - 1 - R.EDGE_AT) for r in sched['probes'] for s, b in sched['backlogs'][r]}
        assert {(62, -1), (64, 0)} <= ends and any(b == 63 and s - b == R.EDGE_AT + 1
                                                    for r in sched['probes'] for s, b in sched['backlogs'][r])
        assert (sched['final'][sched['untouched']] == R.EDGE_STEPS).all()


def test_dup_schedule_places_the_multiplicities():
    us, _ = _schedules(*DUP_CASE, dups=True)
    U = SHAPES[DUP_CASE[0]][0]
    for (k, s), pos in DUP_PLACED.items():
        row, batch = U - N_PROBES + k, us['batches'][s - 1]
        assert np.flatnonzero(batch == row).tolist() == pos
        assert min(pos) % 64 != 0
    assert sorted(len(p) for p in DUP_PLACED.values()) == [2, 9, 10, 70]
    lens = {len(p): dict(us['backlogs'][U - N_PROBES + k])[s] for (k, s), p in DUP_PLACED.items()}
    assert lens == {2: 64, 9: 126, 10: 192, 70: 253}
    pos70 = DUP_PLACED[(8, 259)]
    assert min(pos70) < 64 <= max(pos70)


# ---------------------------------------------------------------------------------------------------
# the restated chain against the oracle's optimiser step (CPU)
# ---------------------------------------------------------------------------------------------------
def _chain_inputs(seed, n):
    rng = np.random.RandomState(seed)
    p = (rng.randn(n) * 0.05).astype(np.float32)
    m = (rng.randn(n) * 1e-3).astype(np.float32)
    v = ((0.25 + rng.rand(n)) * 1e-6).astype(np.float32)
    return p, m, v


def _ratio(err, bound):
    assert (err <= bound).all(), float((err - bound).max())
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


@pytest.mark.parametrize('opt', R.OPTS)
@pytest.mark.parametrize('t0,n', [(0, 300), (R.TAB_LEN - 100, 200)])
def test_chain_agrees_with_the_oracle_step_by_step(oracle, opt, t0, n):
    """zero_grad_chain (float64) against a chain of oracle.opt_step(g = 0) (fp32, torch's operation order) within the
    running rounding bound of replay_restate -- roundings per step x 2^-24 of each quantity's own size."""
    p0, m0, v0 = _chain_inputs(3, 4096)
    p, m, v = p0.copy(), m0.copy(), v0.copy()
    zero = np.zeros_like(p)
    for t in range(t0 + 1, t0 + n + 1):
        oracle.opt_step(opt, p, zero, m, v, LR, WD, t)
        if t in (t0 + 1, t0 + 64, t0 + n):
            rp, rm, rv, Ep, Em, Ev = R.zero_grad_chain_bound(opt, p0, m0, v0, t0, t, LR, WD)
            ratios = (_ratio(np.abs(p - rp), Ep), _ratio(np.abs(v - rv), Ev),
                      _ratio(np.abs(m - rm), Em) if opt != 'adagrad' else 0.0)
            print(f'chain vs oracle {opt} t0={t0} steps={t - t0}: measured/bound p {ratios[0]:.3f} v {ratios[1]:.3f} '
                  f'm {ratios[2]:.3f}')
    if opt == 'adagrad':
        assert np.array_equal(m, m0)
    assert np.abs(p - p0).max() > 50 * Ep.max()      # the chain moved the row by far more than the bound allows to lose


def test_bias_corrections_saturate_long_before_the_table_ends():
    """The replay reads tab[min(t, 65 536)], the eager launch computes its scalars from t: both agree only if the fp32
    scalars have stopped changing by then (hsk_adam_tab_saturates).  Restated from hsk_make_adamw_consts' formula."""
    t = np.arange(1, R.TAB_LEN + 1)
    for lr in (1e-3, LR):
        ss, bs, rbs = R.adam_scalars(lr, t)
        change = (ss[1:] != ss[:-1]) | (bs[1:] != bs[:-1]) | (rbs[1:] != rbs[:-1])
        last = int(t[1:][change].max())
        print(f'lr {lr}: fp32 (step_size, sqrt(bc2), 1/sqrt(bc2)) last change at t = {last}')
        assert last < R.TAB_LEN - 4096
        far = R.adam_scalars(lr, np.array([R.TAB_LEN + 1, 10 ** 6, 2.0 ** 40]))
        for a, b in zip((ss, bs, rbs), far):
            assert (b == a[-1]).all()


# ---------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------
def _tables(shape, bias):
    U, I, D = SHAPES[shape][:3]
    rng = np.random.RandomState(D + U)
    P = {'user_emb': (rng.randn(U, D) * 0.05).astype(np.float32), 'item_emb': (rng.randn(I, D) * 0.05).astype(np.float32),
         'item_bias': (rng.randn(I) * 0.05).astype(np.float32)}
    if bias:
        P['user_bias'] = (rng.randn(U) * 0.05).astype(np.float32)
        P['global_bias'] = np.array([0.03], np.float32)
    M = {k: (rng.randn(*a.shape) * 1e-3).astype(np.float32) for k, a in P.items()}
    V = {k: ((0.25 + rng.rand(*a.shape)) * 1e-6).astype(np.float32) for k, a in P.items()}
    return P, M, V


def _batches(shape, kind, dups=False):
    U, I, D, B, N, _ = SHAPES[shape]
    us, its = _schedules(shape, kind, dups)
    rng = np.random.RandomState(21)
    out = []
    for s, u in enumerate(us['batches']):
        i = its['batches'][s].reshape(B, N + 1) if its else rng.randint(0, I, size=(B, N + 1)).astype(np.int64)
        out.append((u, i))
    return out, us, its


def _preload(st, M, V):
    import torch
    for k in M:
        if st.m[k] is not None:
            st.m[k].copy_(torch.from_numpy(M[k].reshape(-1) if M[k].ndim == 1 else M[k]))
            st.v[k].copy_(torch.from_numpy(V[k].reshape(-1) if V[k].ndim == 1 else V[k]))


def _collect(st, t, losses):
    import torch
    st.flush()
    out = {k: v.cpu() for k, v in t.items()}
    out.update({'m.' + k: v.cpu() for k, v in st.m.items() if v is not None})
    out.update({'v.' + k: v.cpu() for k, v in st.v.items() if v is not None})
    st.check_status()
    return out, torch.stack(losses).cpu().tolist() if losses else []


def _run_eager(ops, tables, batches, K, lazy_users, lazy_items, start, opt, loss='bpr', log_adjust=0.0, apart=False,
               **kw):
    import torch
    from test_hip_parity import _fused_state
    P, M, V = tables
    B = len(batches[0][0])
    st, t = _fused_state(ops, P, LR, WD, B, K, lazy_users=lazy_users, lazy_items=lazy_items, optimizer=opt, loss=loss,
                         log_adjust=log_adjust, flush_every=1 << 20, start_step=start, **kw)
    _preload(st, M, V)
    st.st.catchup_apart = 1 if apart else 0
    uu = torch.from_numpy(np.stack([u for u, _ in batches])).cuda()
    ii = torch.from_numpy(np.stack([i for _, i in batches])).cuda()
    losses = []
    for s in range(len(batches)):
        st.step(uu[s], ii[s])
        losses.append(st.loss_out[0].clone())
    assert st.step_count == start + len(batches)
    cols = st.batch_columns(B, K)
    out, losses = _collect(st, t, losses)
    return out, losses, cols


def _run_oracle(oracle, tables, batches, start, opt, loss='bpr', log_adjust=0.0):
    P, M, V = tables
    tr = oracle.MfOracleTrainer(P['user_emb'], P['item_emb'], P.get('item_bias'), P.get('user_bias'), P.get('global_bias'),
                                lr=LR, wd=WD, loss=loss, log_adjust=log_adjust, optimizer=opt)
    tr.t = start
    for k in tr.P:
        tr.M[k][...] = M[k].reshape(tr.M[k].shape)
        tr.V[k][...] = V[k].reshape(tr.V[k].shape)
    losses = [tr.step(u, i)[0] for u, i in batches]
    return tr, losses


def _assert_bitwise(lazy, dense, l_lazy, l_dense, what):
    import torch
    assert l_lazy == l_dense, what
    assert set(lazy) == set(dense)
    for k in dense:
        assert torch.equal(lazy[k], dense[k]), (what, k, int((lazy[k] != dense[k]).sum()))


def _assert_close_to_oracle(dense, l_dense, tr, l_ref, opt, what):
    for s, (a, b) in enumerate(zip(l_dense, l_ref)):
        assert abs(a - b) <= 1e-6 * abs(b), (what, 'loss', s, a, b)
    max_tol = 5e-3 if opt == 'adagrad' else None      # test_optimizers._max_tol
    for k in tr.P:
        got = dense[k].numpy().reshape(tr.P[k].shape)
        if opt != 'adagrad':
            assert max_norm_err(dense['m.' + k].numpy().reshape(-1), tr.M[k].reshape(-1)) < 1e-5, (what, 'm', k)
        assert max_norm_err(dense['v.' + k].numpy().reshape(-1), tr.V[k].reshape(-1)) < 1e-5, (what, 'v', k)
        assert_adam_param_close(got, tr.P[k], (what, k), max_tol)


def _assert_rows_follow_the_chain(out, tables, key, rows, opt, start, n_steps, what):
    """Rows that only ever saw zero gradients: the lazy run's bits against the float64 chain over the whole run."""
    P, M, V = tables
    sel = (lambda a: a.reshape(len(P[key]), -1)[rows])
    ref = R.zero_grad_chain_bound(opt, sel(P[key]), sel(M[key]), sel(V[key]), start, start + n_steps, LR, WD)
    got = [sel(out[key].numpy()), sel(out['m.' + key].numpy()), sel(out['v.' + key].numpy())]
    ratios = []
    for j, name in enumerate('pmv'):
        err = np.abs(got[j].astype(np.float64) - ref[j])
        assert (err <= ref[3 + j]).all(), (what, key, name, float(err.max()), float(ref[3 + j].max()))
        ratios.append(_ratio(err, ref[3 + j]))
    if opt == 'adagrad':
        assert np.array_equal(got[1], sel(M[key]))
    assert np.abs(ref[0] - sel(P[key])).max() > 50 * ref[3].max(), what      # the bound is far below what the chain moves
    print(f'replay vs chain {what} {key} ({len(rows)} rows, steps {start}+{n_steps}): measured/bound p {ratios[0]:.3f} '
          f'm {ratios[1]:.3f} v {ratios[2]:.3f}')


def _check_case(ops, oracle, shape, kind, start, opt, lazy_items=False, loss='bpr', apart=False, dups=False, bias=True,
                expect_part=False):
    U, I, D, B, N, _ = SHAPES[shape]
    K = N + 1
    what = f'{shape}/{kind}/{start}/{opt}/{loss}'
    tables = _tables(shape, bias)
    batches, us, its = _batches(shape, kind, dups)
    n_steps = len(batches)
    adj = float(np.log(I / N)) if loss == 'sampled_softmax' else 0.0
    lazy, l_lazy, cols = _run_eager(ops, tables, batches, K, True, lazy_items, start, opt, loss, adj, apart)
    dense, l_dense, _ = _run_eager(ops, tables, batches, K, False, False, start, opt, loss, adj)
    assert (cols > K) if expect_part else (cols == K), (what, cols)
    _assert_bitwise(lazy, dense, l_lazy, l_dense, what)
    tr, l_ref = _run_oracle(oracle, tables, batches, start, opt, loss, adj)
    _assert_close_to_oracle(dense, l_dense, tr, l_ref, opt, what)
    _assert_rows_follow_the_chain(lazy, tables, 'user_emb', us['untouched'], opt, start, n_steps, what)
    if bias:     # bpr / sampled softmax: user and global bias have zero gradients by definition, on every row
        _assert_rows_follow_the_chain(lazy, tables, 'user_bias', np.arange(U), opt, start, n_steps, what)
        _assert_rows_follow_the_chain(lazy, tables, 'global_bias', np.arange(1), opt, start, n_steps, what)
    if its is not None:
        _assert_rows_follow_the_chain(lazy, tables, 'item_emb', its['untouched'], opt, start, n_steps, what)
        _assert_rows_follow_the_chain(lazy, tables, 'item_bias', its['untouched'], opt, start, n_steps, what)


@pytest.fixture(scope='module')
def ops():
    from hassaku_amd import hip_ops
    return hip_ops


@pytest.mark.gpu
@pytest.mark.parametrize('shape,opt,loss,kind,start', FORWARD_CASES)
def test_forward_replay_over_long_backlogs(ops, oracle, shape, opt, loss, kind, start):
    """hsk_user_row_current inside the three small-batch forwards, the owners' update from ucur / mcur / vcur, the bias
    scalars' own loops (user_bias, global_bias present) and the closing k_row_flush_wave."""
    _check_case(ops, oracle, shape, kind, start, opt, loss=loss)


@pytest.mark.gpu
def test_partitioned_forward_replay_over_long_backlogs(ops, oracle):
    """k_fwd_part's replay and its hand-over to the owners' update at B = 2048 (P = 2 partitions need >= 16 negatives by
    the partition rule, asserted through batch_columns).  The short plan: every required backlog up to 193 in 200 steps,
    the longest 198; >= 250 is not reached at this batch size."""
    shape, kind, start = PART_CASE
    _check_case(ops, oracle, shape, kind, start, 'adamw', expect_part=True, bias=False)


@pytest.mark.gpu
@pytest.mark.parametrize('shape,opt', APART_CASES)
def test_stand_alone_catch_up_over_long_backlogs(ops, oracle, shape, opt):
    """k_user_catch_up in front of the forward (catchup_apart): one pass of the workgroup at D = 64, the
    hsk_row_replay_wg remainder pass at D = 640 (two floats per thread: 512 + 128).  The library does not report the
    launch: that the flag routes an eager step there is read from hsk_run_step (`apart`), and a mutation of the kernel's
    own loop fails exactly these cases (MEASUREMENTS)."""
    _check_case(ops, oracle, shape, 'long', 0, opt, apart=True)


@pytest.mark.gpu
@pytest.mark.parametrize('opt,kind,start', ITEM_CASES)
def test_lazy_items_over_long_backlogs(ops, oracle, opt, kind, start):
    """k_item_catch_up -- AdamW: the parameter only, the moments brought forward from pend[] by the whole-row item pass;
    adam / adagrad: the full form -- with item probes on the same backlog list, the k_sort_lds touched list."""
    U, I, D, B, N, _ = SHAPES['items']
    assert ops.key_sort_plan(I, B * (N + 1), touched=True)['kind'] == 'lds'
    _check_case(ops, oracle, 'items', kind, start, opt, lazy_items=True)


@pytest.mark.gpu
@pytest.mark.parametrize('shape,opt,kind,start', SWEEP_CASES)
def test_closing_sweep_over_long_backlogs(ops, oracle, shape, opt, kind, start):
    """k_row_flush_wave with three quarters of the rows 200 / 260 steps behind: 1, 2 and 4 floats per lane, whole and
    ragged last chunk, odd D (separate item and user launches)."""
    _check_case(ops, oracle, shape, kind, start, opt)


@pytest.mark.gpu
@pytest.mark.parametrize('opt', ['adamw', 'adagrad'])
def test_duplicate_entries_of_a_row_that_is_behind(ops, oracle, opt):
    """Every further entry of a user replays the same stale row and registers with the owner: 2 and 9 entries (the
    ranked list, 9 = exactly full), 10 (the batch scan), 70 across b = 64 (the scan from the owner's own chunk)."""
    _check_case(ops, oracle, *DUP_CASE, 0, opt, dups=True)


def _beta1_whose_step_size_settles_at_the_table_end():
    """A beta1 for which the fp32 step_size lr / (1 - beta1^t) changes for the last time from t = 65 535 to 65 536: the
    table's last entry is then the only one that holds the saturated value (beta1^t passes the rounding threshold midway
    between the two steps, far from any doubt about pow's last bit)."""
    return float(np.exp(np.log(_step_size_threshold()) / (R.TAB_LEN - 0.5)))


def _step_size_threshold():
    """y below which the double lr / (1 - y) ~ lr (1 + y) rounds to float32(lr): lr (1 + y) < float32(lr) + half an ulp."""
    lr32 = np.float64(np.float32(LR))
    half_ulp = np.float64(np.spacing(np.float32(LR))) / 2
    return (lr32 + half_ulp - LR) / LR


def test_engineered_beta1_puts_the_last_change_at_the_table_end():
    b1 = _beta1_whose_step_size_settles_at_the_table_end()
    t = np.array([R.TAB_LEN - 2, R.TAB_LEN - 1, R.TAB_LEN, R.TAB_LEN + 1, 2.0 ** 40])
    ss, bs, rbs = R.adam_scalars(LR, t, b1=b1)
    assert ss[1] != ss[2] and ss[2] == ss[3] == ss[4] == np.float32(LR), ss
    assert (bs == bs[-1]).all() and (rbs == rbs[-1]).all()       # beta2's corrections settled long before
    y = b1 ** t[1:3]
    assert y[1] < _step_size_threshold() < y[0] and abs(np.log(y[0] * y[1]) / 2 - np.log(_step_size_threshold())) < 1e-9


@pytest.mark.gpu
def test_last_table_entry_is_the_one_used_beyond_the_table(ops):
    """With the beta1 above, entry 65 536 differs from entry 65 535 and equals every later step's scalars: a replay that
    read any other entry beyond the table would leave the dense sweep's bits.  lazy == dense bitwise, and the rows outside
    every batch against the float64 chain (no oracle run: its trainer has the default betas built in)."""
    b1 = _beta1_whose_step_size_settles_at_the_table_end()
    U, I, D, B, N, _ = SHAPES[TABLE_END_CASE[0]]
    tables = _tables(TABLE_END_CASE[0], True)
    batches, us, _ = _batches(*TABLE_END_CASE)
    lazy, l_lazy, _ = _run_eager(ops, tables, batches, N + 1, True, False, EDGE_START, 'adamw', beta1=b1)
    dense, l_dense, _ = _run_eager(ops, tables, batches, N + 1, False, False, EDGE_START, 'adamw', beta1=b1)
    _assert_bitwise(lazy, dense, l_lazy, l_dense, 'beta1')
    P, M, V = tables
    rows = us['untouched']
    ref = R.zero_grad_chain_bound('adamw', P['user_emb'][rows], M['user_emb'][rows], V['user_emb'][rows], EDGE_START,
                                  EDGE_START + len(batches), LR, WD, b1=b1)
    for j, k in enumerate(('user_emb', 'm.user_emb', 'v.user_emb')):
        print(f'beta1 {b1:.8f} {k}: measured/bound', _ratio(np.abs(lazy[k].numpy()[rows].astype(np.float64) - ref[j]), ref[3 + j]))


# ---- the sampled paths: the `order` tensor is the user schedule ---------------------------------------------------
def _sampled_setup(shape, kind):
    U, I, D, B, N, _ = SHAPES[shape]
    us, _ = _schedules(shape, kind)
    rng = np.random.RandomState(31)
    pairs = np.stack([np.repeat(np.arange(U), 6), rng.randint(0, I, size=6 * U)], axis=1)
    pairs = np.unique(pairs, axis=0)
    pairs = pairs[rng.permutation(len(pairs))]
    by_user = np.argsort(pairs[:, 0], kind='stable')            # the interactions grouped by user
    counts = np.bincount(pairs[:, 0], minlength=U)
    assert counts.min() >= 1
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    flat = np.concatenate(us['batches'])
    order = by_user[first[flat] + rng.randint(0, 1 << 30, size=len(flat)) % counts[flat]].astype(np.int64)
    assert np.array_equal(pairs[order, 0].reshape(len(us['batches']), B), np.stack(us['batches']))
    return pairs, order, us


def _run_sampled(ops, tables, pairs, order, shape, lazy, start, mode, n_steps, graph_chunk=-1):
    """mode 'hinted': step_sampled with the next batch named (prefetch; the next batch's rows replayed ahead);
    'single': step_sampled alone; 'run': steps_sampled (replayed graphs with graph_chunk > 0)."""
    import torch
    from test_hip_parity import _fused_state, dev
    U, I, D, B, N, _ = SHAPES[shape]
    P, M, V = tables
    ptr, idx = csr_from_pairs(pairs, U)
    st, t = _fused_state(ops, P, LR, WD, B, N + 1, seed=5, csr_indptr=dev(ptr), csr_indices=dev(idx),
                         coo_user=dev(pairs[:, 0], torch.int32), coo_item=dev(pairs[:, 1], torch.int32),
                         lazy_users=lazy, lazy_items=False, flush_every=1 << 20, start_step=start, graph_chunk=graph_chunk)
    _preload(st, M, V)
    st.st.nnz = len(order)
    od = torch.from_numpy(order).cuda()
    losses, batches = [], []
    if mode == 'run':
        st.steps_sampled(od, 0, n_steps, B, N)
    else:
        for s in range(n_steps):
            if mode == 'hinted' and s + 1 < n_steps:
                st.hint_next(od, (s + 1) * B, B, N)
            st.step_sampled(od, s * B, B, N)
            losses.append(st.loss_out[0].clone())
            if mode == 'single':
                u, i = st.last_batch(B, N + 1)
                batches.append((u, i))
    replays = (st.graph_replays(), st.pipelined_steps())
    loss_sum = st.pop_loss_sum()
    out, losses = _collect(st, t, losses)
    return out, losses, [(u.cpu().numpy(), i.cpu().numpy()) for u, i in batches], replays, loss_sum


@pytest.mark.gpu
@pytest.mark.parametrize('shape,mode,kind,start', SAMPLED_CASES)
def test_sampled_paths_over_long_backlogs(ops, oracle, shape, mode, kind, start):
    """hsk_user_ahead_body -- small batch: the hinted next batch's rows replayed by workgroups of the item launch (64 x 71
    entries, above the prefetch minimum); B = 2048 (the short plan, longest backlog 198): by leading workgroups of the
    partitioned forward in the in-launch pipeline -- and replayed graphs of 16 steps whose kernels take the step from the
    device descriptor.  graph_replays() / pipelined_steps() are asserted for the run modes.  The hinted case has no
    counter to assert: that a hinted batch of >= 4096 entries below B = 2048 gets its rows replayed by the item launch is
    read from hsk_run_step, and a mutation of hsk_user_ahead_body's loop fails it (MEASUREMENTS)."""
    U, I, D, B, N, _ = SHAPES[shape]
    what = f'{shape}/{mode}/{start}'
    tables = _tables(shape, bias=shape != 'part')
    pairs, order, us = _sampled_setup(shape, kind)
    n_steps = len(us['batches'])
    chunk = 16 if shape == 'graph' else -1
    lazy, l_lazy, _, replays, sum_lazy = _run_sampled(ops, tables, pairs, order, shape, True, start, mode, n_steps, chunk)
    dense, l_dense, batches, r0, sum_dense = _run_sampled(ops, tables, pairs, order, shape, False, start, 'single', n_steps)
    assert r0 == (0, 0)
    if mode == 'run':
        if shape == 'graph':
            assert replays == (n_steps // 16, 0)
        else:       # the in-launch pipeline of the partitioned forward
            assert replays[0] == 0 and replays[1] > n_steps // 2, replays
        assert sum_lazy == sum_dense
        l_lazy = l_dense
    _assert_bitwise(lazy, dense, l_lazy, l_dense, what)
    assert all(np.array_equal(u, b) for (u, _), b in zip(batches, us['batches']))
    tr, l_ref = _run_oracle(oracle, tables, batches, start, 'adamw')
    _assert_close_to_oracle(dense, l_dense, tr, l_ref, 'adamw', what)
    _assert_rows_follow_the_chain(lazy, tables, 'user_emb', us['untouched'], 'adamw', start, n_steps, what)
    if 'user_bias' in tables[0]:
        _assert_rows_follow_the_chain(lazy, tables, 'user_bias', np.arange(U), 'adamw', start, n_steps, what)


# ---- k_user_flush: only behind HSK_FLUSH_WAVE=0, which the library reads once per process ---------------------------
def _digests(out, losses):
    d = {k: hashlib.sha256(np.ascontiguousarray(v.numpy()).tobytes()).hexdigest() for k, v in sorted(out.items())}
    d['losses'] = hashlib.sha256(np.asarray(losses, dtype=np.float64).tobytes()).hexdigest()
    return d


def _flush_case(ops, lazy):
    shape = FLUSH_CHILD_CASE[0]
    tables = _tables(shape, True)
    batches, us, _ = _batches(*FLUSH_CHILD_CASE)
    out, losses, _ = _run_eager(ops, tables, batches, SHAPES[shape][4] + 1, lazy, False, 0, 'adamw')
    return out, losses


@pytest.mark.gpu
def test_workgroup_sweep_over_long_backlogs(ops):
    """The closing sweep by k_user_flush (a workgroup per row) in a fresh interpreter with HSK_FLUSH_WAVE=0: digests of
    its lazy run against this process's dense run.  The library does not report which sweep kernel it launched: the
    child asserts that it runs under the switch, hsk_launch_flush reads it once per process, and a mutation of
    hsk_row_replay_wg -- which k_row_flush_wave does not call -- fails this case (MEASUREMENTS)."""
    env = dict(os.environ, HSK_FLUSH_WAVE='0')
    res = subprocess.run([sys.executable, os.path.abspath(__file__), 'flush-child'], env=env, capture_output=True,
                         text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    got = dict(line.split()[1:3] for line in res.stdout.splitlines() if line.startswith('digest '))
    want = _digests(*_flush_case(ops, lazy=False))
    assert got == want, sorted(k for k in want if got.get(k) != want[k])


if __name__ == '__main__' and sys.argv[1:] == ['flush-child']:
    assert os.environ.get('HSK_FLUSH_WAVE') == '0'
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from hassaku_amd import hip_ops as _ops
    for _k, _v in _digests(*_flush_case(_ops, lazy=True)).items():
        print('digest', _k, _v)
